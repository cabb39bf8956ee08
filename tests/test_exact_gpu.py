"""Exact tests of the conv kernels (GPU): `torch.equal` against fp64, no tolerance anywhere in this file.

On the inputs of tests/exact_inputs.py the arithmetic of the kernels is exact in fp32 in any summation order
(tests/test_exact_inputs_host.py proves that on the CPU for every case used here: fp32 in two orders == fp64, and
sum |terms| / u < 2^24 per output element), so the fp64 reference cast to fp32 is THE result and any other bit pattern
is a kernel bug: a voxel dropped from or counted twice in a statistics epilogue (one of P = 50 176 voxels moves a sum of
squares by 2e-5 -- invisible at the 1e-4 of tests/test_ops_gpu.py), one wrong tail tile or M tile diluted by a
whole-tensor norm, a split term lost in a forward kernel (the two-term form sits at 4.4e-6, inside the old 2e-5).

1. integer inputs: outputs AND statistics of every conv entry point, every case of the shared case lists plus large-P rows,
   also under the loop-coverage option grids, bwd_terms 2 / 3 and the fp32-MFMA fallbacks;
2. split-term probes (1 + 2^-10 + 2^-20 against {0, +-1}): every product a three-term kernel keeps is needed to get the
   result; positive control: under bwd_terms = 2 the backward probes that carry a lo term must come out UNEQUAL;
3. operands as the Trainer hands them: parameters, running statistics and weight-gradient outputs as views at unpadded
   (+2, +1, +3 float) offsets inside one NaN-filled flat buffer, bitwise the fresh-tensor call, the rest of the buffer
   untouched;
4. the head GEMMs on integer inputs;
5. mixed storage (bf16 storage of the wide tensors): every entry point that takes `mx`, on hot integer inputs whose bf16 stores
   round -- a bf16 output is bitwise `ref64.float().bfloat16()`, its statistics are bitwise the fp64 sums over the STORED
   tensor; also the BN-finalize forms of the channelwise kernels (dw333_fwd_stats, dw333_bwd(bn=...)) in both storage modes."""
import pytest
import torch

from tests import exact_inputs as ei

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _canary_bands_around_every_output(request):
    """Every KERNEL-LEVEL test of this file runs with guard-band allocation (x3dhip.ops.set_guard): each buffer the ops layer allocates sits
    between two 4 KB canary bands, checked at teardown -- a kernel that writes outside its output at ANY of these shapes
    (odd planes, P % 4 != 0, tail tiles, strided gathers) fails the test even when its own output is right."""
    kernel_level = request.node.name.startswith(("test_pw", "test_dw333", "test_stem", "test_elementwise", "test_head",
                                                 "test_reduce", "test_three_term"))
    if not torch.cuda.is_available() or not kernel_level:
        yield
        return
    from x3dhip import ops
    prev = ops.set_guard(True)
    yield
    torch.cuda.synchronize()
    bad = ops.check_guards()
    ops.set_guard(prev)
    assert not bad, "%d buffers written out of bounds, first: %s" % (len(bad), bad[:6])


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


def _span(v):
    v = sorted(set(int(i) for i in v))
    return "%d" % v[0] if len(v) == 1 else "%d..%d (%d distinct)" % (v[0], v[-1], len(v))


def _where(bad, got, ref):
    """Where a mismatch sits: index ranges per dimension; for [N, C, voxels...] tensors the samples, the 16-row blocks of
    channels and the 32-voxel tiles."""
    idx = bad.nonzero()
    msg = "%d of %d elements differ; " % (idx.shape[0], bad.numel())
    if bad.dim() >= 3:
        flat = bad.flatten(2).nonzero()
        msg += "samples %s, rows %s (16-row blocks %s), voxels %s (32-voxel tiles %s of %d)" % (
            _span(flat[:, 0]), _span(flat[:, 1]), _span(flat[:, 1] // 16), _span(flat[:, 2]), _span(flat[:, 2] // 32),
            -(-bad.flatten(2).shape[2] // 32))
    else:
        msg += ", ".join("dim %d: %s" % (d, _span(idx[:, d])) for d in range(bad.dim()))
    first = [(tuple(int(j) for j in i), float(got[tuple(i)]), float(ref[tuple(i)])) for i in idx[:4]]
    return msg + "; first (index, got, expected): %s" % (first,)


def _eq(got, ref64, what):
    """got (fp32, from the GPU) is bitwise the fp64 reference, which is an fp32 number."""
    ref = ref64.float()
    assert torch.equal(ref.double(), ref64), what + ": the reference is not representable in fp32 (bug in the case)"
    g = got.detach().cpu()
    assert g.dtype == torch.float32 and g.numel() == ref.numel(), (what, g.dtype, tuple(g.shape), tuple(ref.shape))
    g = g.reshape(ref.shape)
    if not torch.equal(g, ref):
        raise AssertionError("%s: %s" % (what, _where(~(g == ref), g, ref)))


def _eq_stats(partial, ref0, ref1, what):
    """Every partial is an exact fp32 number, so the fp64 sum of the partials is the fp64 row sum exactly."""
    st = partial.double().sum(2).cpu()
    for k, ref in ((0, ref0), (1, ref1)):
        g = st[..., k]
        if not torch.equal(g, ref):
            raise AssertionError("%s[%d]: %s" % (what, k, _where(~(g == ref), g, ref)))


def _to(t, dev):
    return None if t is None else t.float().contiguous().to(dev)


BF = torch.bfloat16


def _to_bf(t, dev):
    """A tensor a kernel reads as bf16: the cast must not change a value (tests/test_exact_inputs_host.py proves it does not)."""
    b = t.float().to(BF)
    assert torch.equal(b.double(), t.double()), "not a bf16 tensor (bug in the case)"
    return b.contiguous().to(dev)


def _eq_bf(got, ref64, what):
    """got (bf16, from the GPU) is bitwise the round-to-nearest-even bf16 of the fp64 reference, which is an fp32 number."""
    f = ref64.float()
    assert torch.equal(f.double(), ref64), what + ": the reference is not representable in fp32 (bug in the case)"
    ref = f.to(BF)
    g = got.detach().cpu()
    assert g.dtype == BF and g.numel() == ref.numel(), (what, g.dtype, tuple(g.shape), tuple(ref.shape))
    g = g.reshape(ref.shape)
    if not torch.equal(g, ref):
        raise AssertionError("%s: %s" % (what, _where(~(g == ref), g.float(), ref.float())))


BWD_OPTS = ({}, {"bwd_terms": 2}, {"dgrad_f32": 1, "wgrad_f32": 1})      # integers are pure hi: all exact


# --------------------------------------------------------------------------------------------------- 1. integer inputs
def _pw_forward(ops, c, r, d, what):
    wd = d["w"]
    for wp in (None, ops.pw_pack(wd)):                                   # streaming kernels, then the packed ones
        y, partial = ops.pw_fwd(d["x"], wd, stride=c.s, pre=d["pre"], pre_act=c.act, wp=wp)
        tag = "%s pw_fwd(%s)" % (what, "packed" if wp is not None else "unpacked")
        _eq(y, r["y"], tag + " y")
        _eq_stats(partial, r["sy"], r["sy2"], tag + " statistics")


def _pw_backward(ops, c, r, d, what):
    N, Ci, Co = c.shape[:3]
    g, a, cb, w, x, pre = d["g"], d["a"], d["cb"], d["w"], d["x"], d["pre"]
    dw = ops.pw_bwd_weight(g, a, cb, x, (Co, Ci), stride=c.s, pre=pre, pre_act=c.act)
    _eq(dw, r["dw"], what + " pw_bwd_weight")
    df = ops.DeferredGrads()
    dw = ops.pw_bwd_weight(g, a, cb, x, (Co, Ci), stride=c.s, pre=pre, pre_act=c.act, defer=df)
    df.flush()
    _eq(dw, r["dw"], what + " pw_bwd_weight through DeferredGrads")
    wpt = ops.pw_pack(w, transposed=True)
    if c.s != 1:                                                          # strided forward: dense backward at output resolution
        out, _ = ops.pw_bwd_data(g, a, cb, w, wpt=wpt)
        _eq(out, r["din"], what + " pw_bwd_data (output resolution)")
        return
    for p in (None, wpt):
        tag = "%s (%s)" % (what, "packed" if p is not None else "unpacked")
        out, partial = ops.pw_bwd_data(g, a, cb, w, x=x if c.act else None, pre=pre, pre_act=c.act, addend=d["addend"], wpt=p)
        _eq(out, r["dx_add"], tag + " pw_bwd_data + addend%s" % (" + ReLU backward" if c.act else ""))
        if c.act:
            _eq_stats(partial, r["dx_sg"], r["dx_sgx"], tag + " pw_bwd_data statistics")
        out, _ = ops.pw_bwd_data(g, a, cb, w, addend=d["add2"], addend_stride=2, wpt=p)
        _eq(out, r["dx_add2"], tag + " pw_bwd_data + stride-2 addend")
        for name, add, astride in (("res0", None, 1), ("res1", d["addend"], 1), ("res2", d["add2"], 2)):
            out, partial = ops.pw_bwd_data_res(g, a, cb, w, d["res_out"], d["res_raw"], addend=add, addend_stride=astride, wpt=p)
            _eq(out, r[name], tag + " pw_bwd_data_res " + name)           # (mask zeros included)
            _eq_stats(partial, r[name + "_sg"], r[name + "_sgx"], tag + " pw_bwd_data_res statistics " + name)


def _pw_device(c, dev):
    names = ("x", "w", "pre", "g", "a", "cb") + (("addend", "add2", "res_out", "res_raw") if c.s == 1 else ())
    return {k: _to(getattr(c, k), dev) for k in names}


@pytest.mark.parametrize("case", ei.PW_EXACT)
def test_pw_exact_integers(case):
    """pw_fwd (unpacked and packed), pw_bwd_weight (single and deferred), pw_bwd_data (plain / ReLU backward, dense and
    stride-2 addend), pw_bwd_data_res: outputs and statistics bitwise the fp64 reference; backward under bwd_terms 3 / 2 and
    the fp32-MFMA kernels."""
    from x3dhip import _lib, ops
    dev = _dev()
    c = ei.pw_case(case)
    r = ei.pw_ref(c)
    d = _pw_device(c, dev)
    _pw_forward(ops, c, r, d, "%s" % (case,))
    for opts in BWD_OPTS:
        with _lib.options(**opts):
            _pw_backward(ops, c, r, d, "%s %s" % (case, opts))


@pytest.mark.parametrize("grid", [3, 40])
def test_pw_exact_integers_long_item_loops(grid):
    """The persistent kernels with 3 / 40 workgroups (options pw8_grid, fb_grid: hundreds of items per workgroup, sample
    boundaries inside a walk, buffer parities, tails)."""
    from x3dhip import _lib, ops
    dev = _dev()
    with _lib.options(pw8_grid=grid, pw8_max_k=224, fb_grid=grid):
        for case in ei.PW_GRID:
            c = ei.pw_case(case)
            _pw_forward(ops, c, ei.pw_ref(c), _pw_device(c, dev), "%s grid %d" % (case, grid))
        for case in ei.FUSED_GRID:
            _fused(ops, case, dev, "grid %d" % grid)


@pytest.mark.parametrize("mode", [0, 1, 2, 3])
def test_pw_exact_integers_sixteen_wave_modes(mode):
    """pw6 / pw7 in their 8- and 16-wave forms (option pw_waves16) on the K >= 320 and many-M-tile layers."""
    from x3dhip import _lib, ops
    dev = _dev()
    with _lib.options(pw_waves16=mode, no_pw8=1):
        for case in ei.PW_WAVES16:
            c = ei.pw_case(case)
            r, d = ei.pw_ref(c), _pw_device(c, dev)
            _pw_forward(ops, c, r, d, "%s pw_waves16 %d" % (case, mode))
            _pw_backward(ops, c, r, d, "%s pw_waves16 %d" % (case, mode))


def _fused(ops, case, dev, what="", ga_bf=False):
    """ga_bf: the hot case with g and a handed over as bf16 tensors (X3D_MX_GA); every output is fp32 and keeps its reference."""
    N, Ci, Co, T, H, W, act = case
    P = T * H * W
    mx = ops.MX_GA if ga_bf else 0
    assert ops.pw_bwd_fused_ok(Ci, Co, P, mx=mx)
    c = ei.fused_mx_case(case) if ga_bf else ei.fused_case(case)
    r = ei.fused_ref(c)
    d = {k: _to(getattr(c, k), dev) for k in ("x", "w", "pre", "xo", "ex", "g", "a", "cb", "addend", "add2")}
    if ga_bf:
        d["g"], d["a"] = _to_bf(c.g, dev), _to_bf(c.a, dev)
    wpt = ops.pw_pack(d["w"], transposed=True)
    tag = "%s %s pw_bwd_fused%s" % (case, what, " (g, a bf16)" if ga_bf else "")
    adds = {0: (None, 1), 1: (d["addend"], 1), 2: (d["add2"], 2)}
    for k in (0, 1, 2):                                                   # mode 0: plain (+ addend)
        if not ops.pw_bwd_fused_ok(Ci, Co, P, 0, k != 0, mx):             # (epilogue, addend) pairs the entry point refuses
            continue
        dx, partial, dw = ops.pw_bwd_fused(d["g"], d["a"], d["cb"], (Co, Ci), wpt, d["x"], mode=0, addend=adds[k][0],
                                           addend_stride=adds[k][1])
        assert partial is None
        _eq(dx, r["m0_dx%d" % k], "%s mode 0 dx (addend %d)" % (tag, k))
        _eq(dw, r["m0_dw"], "%s mode 0 dW (addend %d)" % (tag, k))
    if c.act:                                                             # mode 1: ReLU backward of the conv's input
        for k in (0, 2):
            if not ops.pw_bwd_fused_ok(Ci, Co, P, 1, k != 0, mx):
                continue
            dx, partial, dw = ops.pw_bwd_fused(d["g"], d["a"], d["cb"], (Co, Ci), wpt, d["x"], xpre=d["pre"], xact=1, mode=1,
                                               addend=adds[k][0], addend_stride=adds[k][1])
            _eq(dx, r["m1_dx%d" % k], "%s mode 1 dx (addend %d)" % (tag, k))
            _eq(dw, r["m1_dw"], "%s mode 1 dW (addend %d)" % (tag, k))
            _eq_stats(partial, r["m1_dx%d_sg" % k], r["m1_dx%d_sgx" % k], "%s mode 1 statistics (addend %d)" % (tag, k))
    if ops.pw_bwd_fused_ok(Ci, Co, P, 2, True, mx):                        # mode 2: residual-add + ReLU backward
        for k in (1, 2):
            dx, partial, dw = ops.pw_bwd_fused(d["g"], d["a"], d["cb"], (Co, Ci), wpt, d["xo"], mode=2, ex=d["ex"],
                                               addend=adds[k][0], addend_stride=adds[k][1])
            _eq(dx, r["m2_dx%d" % k], "%s mode 2 dx (addend %d)" % (tag, k))
            _eq(dw, r["m2_dw"], "%s mode 2 dW (addend %d)" % (tag, k))
            _eq_stats(partial, r["m2_dx%d_sg" % k], r["m2_dx%d_sgx" % k], "%s mode 2 statistics (addend %d)" % (tag, k))


@pytest.mark.parametrize("terms", [3, 2])
@pytest.mark.parametrize("case", ei.FUSED_EXACT)
def test_pw_exact_integers_bwd_fused(case, terms):
    """x3d_pw_bwd_fused modes 0 / 1 / 2, dense and stride-2 addend: dx, dW and the statistics bitwise the fp64 reference."""
    from x3dhip import _lib, ops
    dev = _dev()
    with _lib.options(bwd_terms=terms):
        _fused(ops, case, dev, "terms %d" % terms)


def _dw(ops, c, r, d, what):
    y, partial = ops.dw333_fwd(d["x"], d["w"], stride=c.s, pre=d["pre"], pre_act=1)
    _eq(y, r["y"], what + " dw333_fwd y")
    _eq_stats(partial, r["sy"], r["sy2"], what + " dw333_fwd statistics")
    out, dw, bp = ops.dw333_bwd(d["g"], d["a"], d["cb"], d["w"], d["x"], stride=c.s, pre=d["pre"], pre_act=1)
    _eq(out, r["dx"], what + " dw333_bwd dx")
    _eq(dw, r["dw"], what + " dw333_bwd dw")
    _eq_stats(bp, r["sg"], r["sgx"], what + " dw333_bwd statistics")


@pytest.mark.parametrize("case", ei.DW_EXACT)
def test_dw333_exact_integers(case):
    """dw333_fwd / dw333_bwd: y, dx, dw and both statistics bitwise the fp64 reference; for T >= 8 also with the T march cut
    in two (and four, T >= 16) segments (options dw_tsplit_wgs[_fwd], dw_tquad_wgs[_fwd] forced on)."""
    from x3dhip import _lib, ops
    dev = _dev()
    c = ei.dw_case(case)
    r = ei.dw_ref(c)
    d = {k: _to(getattr(c, k), dev) for k in ("x", "w", "pre", "g", "a", "cb")}
    _dw(ops, c, r, d, "%s" % (case,))
    T = case[2]
    if T >= 8:
        for quad in ((0, 1 << 20) if T >= 16 else (0,)):
            with _lib.options(dw_tsplit_wgs=1 << 20, dw_tsplit_wgs_fwd=1 << 20, dw_tquad_wgs=quad, dw_tquad_wgs_fwd=quad):
                _dw(ops, c, r, d, "%s T segments (quad %d)" % (case, quad))


@pytest.mark.parametrize("case", ei.DW_TSEG)
def test_dw333_exact_integers_t_segments(case):
    """The remaining shapes of test_dw333_t_segments_equal_the_single_march, unsplit and with the T march forced into
    segments: with exact arithmetic the statistics and dw are bitwise too (there: 1e-6)."""
    from x3dhip import _lib, ops
    dev = _dev()
    c = ei.dw_case(case)
    r = ei.dw_ref(c)
    d = {k: _to(getattr(c, k), dev) for k in ("x", "w", "pre", "g", "a", "cb")}
    _dw(ops, c, r, d, "%s" % (case,))
    for quad in ((0, 1 << 20) if case[2] >= 16 else (0,)):
        with _lib.options(dw_tsplit_wgs=1 << 20, dw_tsplit_wgs_fwd=1 << 20, dw_tquad_wgs=quad, dw_tquad_wgs_fwd=quad):
            _dw(ops, c, r, d, "%s T segments (quad %d)" % (case, quad))


@pytest.mark.parametrize("shape", ei.STEM_EXACT)
def test_stem_exact_integers(shape):
    """stem133_fwd, dw5t_fwd (+ statistics), dw5t_bwd (dx, dw), stem133_bwd_weight bitwise the fp64 reference."""
    from x3dhip import ops
    _stem(ops, shape, _dev())


def _stem(ops, shape, dev, what=""):
    c = ei.stem_case(shape)
    r = ei.stem_ref(c)
    x, ws, wt, g, a, cb = (_to(getattr(c, k), dev) for k in ("x", "ws", "wt", "g", "a", "cb"))
    what = "%s%s" % (shape, what)
    ys = ops.stem133_fwd(x, ws)
    _eq(ys, r["ys"], what + " stem133_fwd")
    yt, partial = ops.dw5t_fwd(_to(r["ys"], dev), wt)
    _eq(yt, r["yt"], what + " dw5t_fwd y")
    _eq_stats(partial, r["sy"], r["sy2"], what + " dw5t_fwd statistics")
    dys, dwt = ops.dw5t_bwd(g, a, cb, wt, _to(r["ys"], dev))
    _eq(dys, r["dys"], what + " dw5t_bwd dx")
    _eq(dwt, r["dwt"], what + " dw5t_bwd dw")
    dws = ops.stem133_bwd_weight(x, _to(r["dys"], dev), ws.shape)
    _eq(dws, r["dws"], what + " stem133_bwd_weight")


# --------------------------------------------------------------------------------------------------- 4. head GEMMs
@pytest.mark.parametrize("R", ei.HEAD_R)
def test_head_exact_integers(R):
    """head_fwd (p = 0) and head_bwd on integer inputs, K in {48, 432, 630, 640} x C in {1, 10, 157, 400} (class-slice tails:
    C < 16, C % 16 != 0): hidden, logits, dW1, dW2, db2, dpooled bitwise the fp64 reference."""
    from x3dhip import ops
    dev = _dev()
    for (r_, K, J, C) in ei.HEAD_EXACT:
        if r_ != R:
            continue
        c = ei.head_case(R, K, J, C)
        r = ei.head_ref(c)
        pooled, w1, w2, b2, dlg = (_to(getattr(c, k), dev) for k in ("pooled", "w1", "w2", "b2", "dlg"))
        what = "head %s" % ((R, K, J, C),)
        hd, logits = ops.head_fwd(pooled, w1, w2, b2, 0.0, None)
        _eq(hd, r["hidden"], what + " hidden")
        _eq(logits, r["logits"], what + " logits")
        dpooled, dw1, dw2, db2 = ops.head_bwd(dlg, _to(r["hidden"], dev), pooled, w1, w2, 0.0)
        _eq(dw1, r["dw1"], what + " dW1")
        _eq(dw2, r["dw2"], what + " dW2")
        _eq(db2, r["db2"], what + " db2")
        _eq(dpooled, r["dpooled"], what + " dpooled")


# --------------------------------------------------------------------------------------------------- 2. split-term probes
def _unit_cb(N, C, dev):
    """dY = 1 g + 0 a + 0: the upstream gradient passes the BN-backward combine unchanged."""
    cb = torch.zeros(N, C, 3, device=dev)
    cb[..., 0] = 1.0
    return cb


@pytest.mark.parametrize("kind", ei.PROBE_KINDS)
@pytest.mark.parametrize("kernel,shape,opts", [(k, s, o) for k, v in ei.PROBE_FWD.items() for s in v
                                               for o in ([{}] if k != "pw6_kernel" else
                                                         [{"no_pw8": 1}, {"no_pw8": 1, "pw_waves16": 0}] if s[1] >= 320 else [{"no_pw8": 1}])])
def test_pw_probe_forward_keeps_every_split_term(kernel, shape, opts, kind):
    """pw6_kernel (8- and 16-wave forms), pw8_kernel, pw_fwd_stream_kernel: y bitwise the fp64 result of a probe that needs
    hi.lo / hi.mid (probe on the activations), lo.hi / mid.hi (on the weights) or mid.mid (both)."""
    from x3dhip import _lib, ops
    dev = _dev()
    w, x, y = ei.probe_fwd(shape, kind)
    wd = _to(w, dev)
    with _lib.options(**opts):
        y_h, _ = ops.pw_fwd(_to(x, dev), wd, wp=ops.pw_pack(wd))
        k = _lib.last_kernel()
    assert k == kernel, (k, kernel)
    _eq(y_h, y, "%s %s probe on %s" % (kernel, shape, kind))


def _lo_control(got, ref64, kind, what):
    """Positive control (bwd_terms = 2): a probe that carries a lo term must NOT come out right without it."""
    if kind in ei.CARRIES_LO:
        assert not torch.equal(got.detach().cpu().reshape(ref64.shape), ref64.float()), \
            what + ": equal to the reference WITHOUT the lo term -- the probe does not reach it"


@pytest.mark.parametrize("kind", ei.PROBE_KINDS)
@pytest.mark.parametrize("shape", ei.PROBE_DGRAD)
def test_pw_probe_data_gradient_keeps_every_split_term(shape, kind):
    """pw7_kernel (pw_bwd_data) and pw7r_kernel (pw_bwd_data_res, mask all ones)."""
    from x3dhip import _lib, ops
    dev = _dev()
    N, Ci, Co, T, H, W = shape
    w, dY, dX = ei.probe_dgrad(shape, kind)
    wd, g = _to(w, dev), _to(dY, dev)
    a, cb = torch.zeros_like(g), _unit_cb(N, Co, dev)
    wpt = ops.pw_pack(wd, transposed=True)
    ones, zeros = torch.ones(N, Ci, T, H, W, device=dev), torch.zeros(N, Ci, T, H, W, device=dev)
    for terms in (3, 2):
        with _lib.options(bwd_terms=terms):
            o7, _ = ops.pw_bwd_data(g, a, cb, wd, wpt=wpt)
            k7 = _lib.last_kernel()
            o7r, _ = ops.pw_bwd_data_res(g, a, cb, wd, ones, zeros, wpt=wpt)
            k7r = _lib.last_kernel()
        assert (k7, k7r) == ("pw7_kernel", "pw7r_kernel"), (k7, k7r)
        for name, o in (("pw7_kernel", o7), ("pw7r_kernel", o7r)):
            what = "%s %s probe on %s, %d terms" % (name, shape, kind, terms)
            if terms == 3:
                _eq(o, dX, what)
            else:
                _lo_control(o, dX, kind, what)


@pytest.mark.parametrize("kind", ei.PROBE_KINDS)
@pytest.mark.parametrize("shape", ei.PROBE_FUSED)
def test_pw_probe_bwd_fused_keeps_every_split_term(shape, kind):
    """pw_bwd_fused_kernel: one launch probes the data-gradient GEMM (x = 0), a second one the weight-gradient GEMM (w = 0)."""
    from x3dhip import _lib, ops
    dev = _dev()
    N, Ci, Co, T, H, W = shape
    assert ops.pw_bwd_fused_ok(Ci, Co, T * H * W)
    w, dY, dX = ei.probe_dgrad(shape, kind)
    dY2, x2, dW = ei.probe_wgrad(shape, kind)
    cb = _unit_cb(N, Co, dev)
    zx, zw = torch.zeros(N, Ci, T, H, W, device=dev), torch.zeros(Co, Ci, device=dev)
    for terms in (3, 2):
        with _lib.options(bwd_terms=terms):
            g = _to(dY, dev)
            dx, _, dw0 = ops.pw_bwd_fused(g, torch.zeros_like(g), cb, (Co, Ci), ops.pw_pack(_to(w, dev), transposed=True), zx, mode=0)
            k = _lib.last_kernel()
            g2 = _to(dY2, dev)
            dx0, _, dw = ops.pw_bwd_fused(g2, torch.zeros_like(g2), cb, (Co, Ci), ops.pw_pack(zw, transposed=True), _to(x2, dev), mode=0)
        assert k == "pw_bwd_fused_kernel", k
        what = "pw_bwd_fused_kernel %s probe on %s, %d terms" % (shape, kind, terms)
        _eq(dw0, torch.zeros(Co, Ci, dtype=torch.float64), what + " dW of x = 0")
        _eq(dx0, torch.zeros(N, Ci, T, H, W, dtype=torch.float64), what + " dx of w = 0")
        if terms == 3:
            _eq(dx, dX, what + " dx")
            _eq(dw, dW, what + " dW")
        else:
            _lo_control(dx, dX, kind, what + " dx")
            _lo_control(dw, dW, kind, what + " dW")


@pytest.mark.parametrize("kind", ei.PROBE_KINDS)
@pytest.mark.parametrize("shape", ei.PROBE_WGRAD)
def test_pw_probe_weight_gradient_keeps_every_split_term(shape, kind):
    """pw_wgrad3_kernel (single launch) and the batched kernels behind DeferredGrads (pw_wgrad3_batch_kernel, and the wide-tile
    pw_wgrad4_batch_kernel where Cout > 128 with Cin > 64)."""
    from x3dhip import _lib, ops
    dev = _dev()
    N, Ci, Co, T, H, W = shape
    dY, x, dW = ei.probe_wgrad(shape, kind)
    g, xd = _to(dY, dev), _to(x, dev)
    a, cb = torch.zeros_like(g), _unit_cb(N, Co, dev)
    wide = (Co > 128 and Ci > 64) or (Co > 64 and Ci > 128)
    for terms in (3, 2):
        with _lib.options(bwd_terms=terms):
            d1 = ops.pw_bwd_weight(g, a, cb, xd, (Co, Ci))
            k1 = _lib.last_kernel()
            df = ops.DeferredGrads()
            d2 = ops.pw_bwd_weight(g, a, cb, xd, (Co, Ci), defer=df)
            df.flush()
            k2 = _lib.last_kernel()
        assert k1 == "pw_wgrad3_kernel", k1
        assert k2 == ("pw_wgrad4_batch_kernel" if wide else "pw_wgrad3_batch_kernel"), (k2, wide)
        for name, o in ((k1, d1), (k2, d2)):
            what = "%s %s probe on %s, %d terms" % (name, shape, kind, terms)
            if terms == 3:
                _eq(o, dW, what)
            else:
                _lo_control(o, dW, kind, what)


# --------------------------------------------------------------------------------------------------- 3. Trainer-like operands
_NAN = float("nan")


def _bits(t):
    return t.detach().contiguous().view(torch.int32).cpu()


def _as_the_trainer_hands_them(dev, fn, params, what):
    """fn(p) -> tensors, with p = {name: device tensor} the parameters / running statistics / gradient outputs of one entry
    point (gradient outputs start as NaN unless given values).  Runs fn on fresh (256-byte aligned) tensors and on the same
    values as views into one flat NaN-filled buffer at unpadded offsets (+2, +1, +3, +2, ... floats modulo 4, as FlatParams
    places them) and requires bitwise equal results, bitwise equal final contents of every p, and every other element of the
    flat buffer still NaN."""
    names = list(params)
    fresh = {k: params[k].detach().clone().float().contiguous().to(dev) for k in names}
    r0 = [t.clone() for t in fn(fresh)]
    want = (2, 1, 3)
    offs, off = {}, 0
    for i, k in enumerate(names):
        off += 4 + (want[i % 3] - off) % 4                               # at least 4 NaN floats between neighbours
        offs[k] = off
        off += params[k].numel()
    flat = torch.full((off + 7,), _NAN, device=dev)
    assert flat.data_ptr() % 16 == 0
    views = {}
    for k in names:
        v = flat[offs[k]:offs[k] + params[k].numel()].view(params[k].shape)
        v.copy_(params[k].float())
        assert v.data_ptr() % 16 != 0 and v.is_contiguous()
        views[k] = v
    r1 = fn(views)
    torch.cuda.synchronize()
    assert len(r0) == len(r1)
    for i, (u, v) in enumerate(zip(r0, r1)):
        assert torch.equal(_bits(u), _bits(v)), "%s: result %d differs between fresh tensors and flat-buffer views" % (what, i)
    for k in names:
        assert torch.equal(_bits(fresh[k]), _bits(views[k])), "%s: %s differs after the call" % (what, k)
    covered = torch.zeros(flat.numel(), dtype=torch.bool)
    for k in names:
        covered[offs[k]:offs[k] + params[k].numel()] = True
    stray = (~torch.isnan(flat.cpu())) & ~covered
    assert not bool(stray.any()), "%s: flat buffer written outside the operands at %s" % (what, stray.nonzero().flatten()[:8].tolist())


def _rn(*shape, seed=0, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


def _nan(*shape):
    return torch.full(shape, _NAN)


@pytest.mark.parametrize("case", [(2, 24, 54, 4, 6, 6, 1), (2, 54, 24, 4, 6, 6, 1), (2, 96, 216, 2, 6, 6, 1), (2, 432, 192, 2, 5, 5, 1),
                                  (1, 70, 98, 2, 6, 6, 1), (1, 24, 54, 2, 9, 7, 1), (2, 48, 96, 4, 8, 8, 2)])
def test_pw_operands_as_flat_buffer_views(case):
    """Pointwise weights (read directly and as the source of both packs) and weight-gradient outputs (out= single and deferred,
    dw_out= of the fused kernel)."""
    from x3dhip import ops
    dev = _dev()
    N, Ci, Co, T, H, W, s = case
    Ho, Wo = ei.out_hw(H, s), ei.out_hw(W, s)
    x = _rn(N, Ci, T, H, W, seed=1).to(dev)
    pre = torch.stack([1 + 0.2 * _rn(N, Ci, seed=3), 0.3 * _rn(N, Ci, seed=4)], -1).contiguous().to(dev)
    g, a = _rn(N, Co, T, Ho, Wo, seed=5).to(dev), _rn(N, Co, T, Ho, Wo, seed=6).to(dev)
    cb = torch.stack([1 + 0.1 * _rn(N, Co, seed=7), 0.1 * _rn(N, Co, seed=8), 0.05 * _rn(N, Co, seed=9)], -1).contiguous().to(dev)
    fused = s == 1 and ops.pw_bwd_fused_ok(Ci, Co, T * Ho * Wo)

    def fn(p):
        w = p["w"]
        wp, wpt = ops.pw_pack(w), ops.pw_pack(w, transposed=True)
        outs = [wp, wpt]
        outs += list(ops.pw_fwd(x, w, stride=s, pre=pre, pre_act=1))
        outs += list(ops.pw_fwd(x, w, stride=s, pre=pre, pre_act=1, wp=wp))
        outs.append(ops.pw_bwd_data(g, a, cb, w)[0])
        outs.append(ops.pw_bwd_data(g, a, cb, w, wpt=wpt)[0])
        ops.pw_bwd_weight(g, a, cb, x, (Co, Ci), stride=s, pre=pre, pre_act=1, out=p["dw"].view(-1))
        df = ops.DeferredGrads()
        ops.pw_bwd_weight(g, a, cb, x, (Co, Ci), stride=s, pre=pre, pre_act=1, out=p["dw_deferred"].view(-1), defer=df)
        df.flush()
        if fused:
            dx, _, _ = ops.pw_bwd_fused(g, a, cb, (Co, Ci), wpt, x, mode=0, dw_out=p["dw_fused"].view(-1))
            outs.append(dx)
        return outs

    params = {"w": _rn(Co, Ci, seed=2, scale=Ci ** -0.5), "dw": _nan(Co, Ci), "dw_deferred": _nan(Co, Ci)}
    if fused:
        params["dw_fused"] = _nan(Co, Ci)
    _as_the_trainer_hands_them(dev, fn, params, "pointwise %s" % (case,))


@pytest.mark.parametrize("case", [(2, 6, 4, 14, 14, 1), (1, 5, 5, 13, 9, 1), (2, 4, 4, 16, 16, 2), (1, 33, 2, 4, 4, 2), (2, 54, 2, 8, 8, 1)])
def test_dw333_operands_as_flat_buffer_views(case):
    """Depthwise weights and their gradient; gamma / beta / running statistics of the finalize folded into the forward
    prologue; gamma / dgamma / dbeta of the one folded into the backward prologue."""
    from x3dhip import ops
    dev = _dev()
    N, C, T, H, W, s = case
    Ho, Wo = ei.out_hw(H, s), ei.out_hw(W, s)
    x = _rn(N, C, T, H, W, seed=1).to(dev)
    pre = torch.stack([1 + 0.2 * _rn(N, C, seed=3), 0.3 * _rn(N, C, seed=4)], -1).contiguous().to(dev)
    g, a = _rn(N, C, T, Ho, Wo, seed=5).to(dev), _rn(N, C, T, Ho, Wo, seed=6).to(dev)
    cb = torch.stack([1 + 0.1 * _rn(N, C, seed=7), 0.1 * _rn(N, C, seed=8), 0.05 * _rn(N, C, seed=9)], -1).contiguous().to(dev)
    sp = torch.stack([_rn(N, C, 5, seed=11) * 3, 50 + _rn(N, C, 5, seed=12).abs() * 40], -1).contiguous().to(dev)
    spb = torch.stack([_rn(N, C, 5, seed=13), 2 * _rn(N, C, 5, seed=14)], -1).contiguous().to(dev)
    save = torch.stack([0.1 * _rn(1, C, seed=15), 1 + 0.1 * _rn(1, C, seed=16).abs()], 0).contiguous().to(dev)
    P, Po = T * H * W, T * Ho * Wo

    def fn(p):
        outs = list(ops.dw333_fwd(x, p["w"], stride=s, pre=pre, pre_act=1))
        outs += list(ops.dw333_fwd_stats(x, p["w"], sp, 1, P, p["gamma"], p["beta"], p["rm"], p["rv"], stride=s, pre_act=1))
        o, _, bp = ops.dw333_bwd(g, a, cb, p["w"], x, stride=s, pre=pre, pre_act=1, dw_out=p["dw"].view(-1))
        outs += [o, bp]
        o, _, bp = ops.dw333_bwd(g, a, None, p["w"], x, stride=s, pre=pre, pre_act=1, dw_out=p["dw_bn"].view(-1),
                                 bn=(spb, Po, p["gamma"], save, p["dgamma"], p["dbeta"]))
        return outs + [o, bp]

    params = {"w": _rn(C, 1, 3, 3, 3, seed=2, scale=1 / 3), "gamma": 1 + 0.2 * _rn(C, seed=17), "beta": 0.3 * _rn(C, seed=18),
              "rm": 0.1 * _rn(1, C, seed=19), "rv": 1 + 0.1 * _rn(1, C, seed=20).abs(), "dw": _nan(C, 1, 3, 3, 3),
              "dw_bn": _nan(C, 1, 3, 3, 3), "dgamma": _nan(C), "dbeta": _nan(C)}
    _as_the_trainer_hands_them(dev, fn, params, "dw333 %s" % (case,))


@pytest.mark.parametrize("shape", [(2, 3, 4, 16, 16), (1, 3, 3, 15, 11), (2, 3, 5, 17, 23)])
def test_stem_operands_as_flat_buffer_views(shape):
    from x3dhip import ops
    dev = _dev()
    N, Ci, T, H, W = shape
    Co = 24
    x = _rn(*shape, seed=1).to(dev)
    Ho, Wo = ei.out_hw(H, 2), ei.out_hw(W, 2)
    g, a = _rn(N, Co, T, Ho, Wo, seed=5).to(dev), _rn(N, Co, T, Ho, Wo, seed=6).to(dev)
    cb = torch.stack([1 + 0.1 * _rn(N, Co, seed=7), 0.1 * _rn(N, Co, seed=8), 0.05 * _rn(N, Co, seed=9)], -1).contiguous().to(dev)

    def fn(p):
        ys = ops.stem133_fwd(x, p["ws"])
        yt, partial = ops.dw5t_fwd(ys, p["wt"])
        dys, _ = ops.dw5t_bwd(g, a, cb, p["wt"], ys, dw_out=p["dwt"].view(-1))
        ops.stem133_bwd_weight(x, dys, p["ws"].shape, out=p["dws"].view(-1))
        return [ys, yt, partial, dys]

    params = {"ws": _rn(Co, Ci, 1, 3, 3, seed=2, scale=0.2), "wt": _rn(Co, 1, 5, 1, 1, seed=3, scale=0.5),
              "dws": _nan(Co, Ci, 1, 3, 3), "dwt": _nan(Co, 1, 5, 1, 1)}
    _as_the_trainer_hands_them(dev, fn, params, "stem %s" % (shape,))


@pytest.mark.parametrize("case", [(8, 54, 8, 4, 1), (8, 108, 8, 65, 1), (8, 216, 16, 98, 1), (8, 432, 32, 25, 1), (16, 216, 16, 49, 2),
                                  (4, 630, 40, 25, 2), (3, 70, 7, 13, 3), (2, 306, 20, 5, 1), (2, 1024, 64, 30, 1)])
def test_elementwise_bn_se_operands_as_flat_buffer_views(case):
    """gamma / beta / running statistics of the finalize kernels (plain, folded into the residual epilogue, eval
    coefficients), SE w1 b1 w2 b2 (Wd % 4 == 0: the float4 fc2 loads) and the gradient outputs of the backward finalizes."""
    from x3dhip import _lib, ops
    dev = _dev()
    N, C, Wd, tiles, S = case
    count = 32 * tiles
    sp = torch.stack([_rn(N, C, tiles, seed=21) * 30, 800 + _rn(N, C, tiles, seed=22).abs() * 400], -1).contiguous().to(dev)
    part = torch.stack([_rn(N, C, tiles, seed=31) * 0.3, _rn(N, C, tiles, seed=32) * 2], -1).contiguous().to(dev)
    save = torch.stack([0.2 * _rn(S, C, seed=35), 0.5 + _rn(S, C, seed=36).abs()], 0).contiguous().to(dev)
    nsum = (_rn(N, C, seed=37) * count * 0.3).to(dev)
    se = torch.sigmoid(_rn(N, C, seed=40)).to(dev)
    z = torch.relu(_rn(N, Wd, seed=41)).to(dev)
    pool = _rn(N, C, seed=42).to(dev)
    a3, res = _rn(N, C, count, 1, 1, seed=43).to(dev), _rn(N, C, count, 1, 1, seed=44).to(dev)

    def fn(p):
        outs = []
        rm, rv = p["rm"], p["rv"]
        coef, sv, ns = ops.bn_fwd_finalize(sp, S, count, p["gamma"], p["beta"], rm, rv, 0.1, 1e-5, want_nsum=True)
        outs += [coef, sv, ns]
        outs += list(ops.se_fwd(coef, ns, count, p["w1"], p["b1"], p["w2"], p["b2"]))
        outs += list(ops.se_bn_fwd(sp, S, count, p["gamma"], p["beta"], rm, rv, p["w1"], p["b1"], p["w2"], p["b2"], 0.1, 1e-5))
        outs += list(ops.bn_stats_add_relu_fwd(a3, sp, S, count, p["gamma"], p["beta"], rm, rv, res))
        outs.append(ops.bn_eval_coef(rm[0], rv[0], p["gamma"], p["beta"], N))
        cbv, _, _ = ops.bn_bwd_finalize(part, S, count, p["gamma"], save, dgamma=p["dgamma"], dbeta=p["dbeta"])
        outs.append(cbv)
        for merge, tag in ((0, "m"), (1, "u")):
            with _lib.options(no_se_bwd_merge=merge):
                cb2, _ = ops.se_bn_bwd_finalize(part, S, count, p["gamma"], p["beta"], save, nsum, p["w1"], p["w2"], se, z, pool,
                                                outs={k: p["se_%s_%s" % (tag, k)] for k in ("dgamma", "dbeta", "dw1", "db1", "dw2", "db2")})
            outs.append(cb2)
        return outs

    params = {"gamma": 1 + 0.2 * _rn(C, seed=23), "beta": 0.3 * _rn(C, seed=24), "rm": 0.1 * _rn(S, C, seed=29),
              "rv": 1 + 0.1 * _rn(S, C, seed=30).abs(), "w1": _rn(Wd, C, seed=25, scale=C ** -0.5), "b1": 0.1 * _rn(Wd, seed=26),
              "w2": _rn(C, Wd, seed=27, scale=Wd ** -0.5), "b2": 0.1 * _rn(C, seed=28), "dgamma": _nan(C), "dbeta": _nan(C)}
    for tag in ("m", "u"):
        params.update({"se_%s_dgamma" % tag: _nan(C), "se_%s_dbeta" % tag: _nan(C), "se_%s_dw1" % tag: _nan(Wd, C),
                       "se_%s_db1" % tag: _nan(Wd), "se_%s_dw2" % tag: _nan(C, Wd), "se_%s_db2" % tag: _nan(C)})
    _as_the_trainer_hands_them(dev, fn, params, "BN / SE %s" % (case,))


@pytest.mark.parametrize("R,K,J,C", [(8, 432, 2048, 400), (3, 630, 2048, 157), (9, 48, 64, 10), (70, 640, 2048, 1)])
def test_head_operands_as_flat_buffer_views(R, K, J, C):
    """Head w1 / w2 / b2 and their gradients (outs=)."""
    from x3dhip import ops
    dev = _dev()
    pooled = torch.relu(_rn(R, K, seed=1)).to(dev)
    dlg = _rn(R, C, seed=5).to(dev)

    def fn(p):
        hd, logits = ops.head_fwd(pooled, p["w1"], p["w2"], p["b2"], 0.0, None)
        dpooled, _, _, _ = ops.head_bwd(dlg, hd, pooled, p["w1"], p["w2"], 0.0, outs=(p["dw1"], p["dw2"], p["db2"]))
        return [hd, logits, dpooled]

    params = {"w1": _rn(J, K, seed=2, scale=K ** -0.5), "w2": _rn(C, J, seed=3, scale=J ** -0.5), "b2": 0.1 * _rn(C, seed=4),
              "dw1": _nan(J, K), "dw2": _nan(C, J), "db2": _nan(C)}
    _as_the_trainer_hands_them(dev, fn, params, "head %s" % ((R, K, J, C),))


@pytest.mark.parametrize("n", [1, 3, 255, 256, 257, 1000, 4098, 100003])
def test_elementwise_sgd_and_grad_accumulate_on_flat_buffer_ranges(n):
    """x3d_sgd_fused / x3d_grad_accumulate on ranges that start at unpadded offsets of the flat parameter / gradient /
    momentum buffers."""
    from x3dhip import ops
    dev = _dev()

    def fn(p):
        ops.grad_accumulate(p["acc"], p["g"], 0.5, True)
        ops.grad_accumulate(p["acc"], p["g"], 0.25, False)
        ops.sgd_fused(p["w"], p["acc"], p["m"], 0.1, first=True)
        ops.sgd_fused(p["w"], p["g"], p["m"], 0.1, grad_scale=0.5, first=False)
        return []

    params = {"w": _rn(n, seed=1), "g": _rn(n, seed=2), "acc": _nan(n), "m": _nan(n)}
    _as_the_trainer_hands_them(dev, fn, params, "sgd / accumulate n = %d" % n)


# --------------------------------------------------------------------------------------------------- 5. mixed storage
# bf16 storage of the wide tensors (include/x3dhip.h X3D_MX_*) on the HOT integer inputs of tests/exact_inputs.py, whose bf16
# stores really round (ties both ways, non-ties both ways; tests/test_exact_inputs_host.py proves it per case and shows that a
# truncating store, a store rounding half away from zero and statistics taken before the store all differ from these
# references).  A bf16 output is compared with `ref64.float().bfloat16()`, the statistics that describe it with the fp64 sums
# over THAT tensor, everything else with the fp32 case's reference.  Entry point (flags its header comment admits) -> test:
#   x3d_pw_fwd             X, Y, X|Y (packed weights); y and statistics          test_pw_exact_mx
#   x3d_pw_bwd_data        GA (dense / stride-2 addend, ReLU backward);
#                          X|Y and GA|X|Y with ReLU backward; out and statistics test_pw_exact_mx
#   x3d_pw_bwd_data_res    GA; three addend forms; out and statistics            test_pw_exact_mx
#   x3d_pw_bwd_weight      GA, X, GA|X; single and through DeferredGrads
#   (x3d_pw_bwd_weight_batch)                                                    test_pw_exact_mx
#   x3d_pw_bwd_fused       GA in modes 0 / 1 / 2 (all addend forms); X|Y in
#                          mode 1; dx, dW, statistics                            test_pw_exact_mx_bwd_fused
#   x3d_pw_fwd, x3d_pw_bwd_fused   persistent loops on 3 / 40 workgroups         test_pw_exact_mx_long_item_loops
#   x3d_dw333_fwd          X|Y                                                   test_dw333_exact_mx
#   x3d_dw333_bwd          GA|X|Y; dx, dw, statistics                            test_dw333_exact_mx
#   x3d_dw333_fwd_stats    0 and X|Y; y, statistics, coef, save, running stats   test_dw333_exact_bn_forms
#   x3d_dw333_bwd_stats    0 and GA|X|Y; dx, dw, statistics, dgamma, dbeta       test_dw333_exact_bn_forms
#   x3d_pw_bwd_tiles, x3d_pw_bwd_fused_ok   (queries with the call's mx)         asked by the ops layer in every call above
# The backward entry points of the pointwise convs run under bwd_terms 3 and 2 (exact either way: dY is hi + mid, every other
# operand pure hi).
MX_BWD_OPTS = ({}, {"bwd_terms": 2})
# the kernel a case must land on in the mixed mode: (forward, data gradient).  * = another kernel than the fp32 mode runs
_S, _P3, _P6, _P7 = "pw_fwd_stream_kernel", "pw3_kernel", "pw6_kernel", "pw7_kernel"
MX_KERNELS = {(2, 24, 54, 4, 16, 16, 1): (_S, _P3), (2, 54, 24, 4, 16, 16, 1): (_P3, _P3), (2, 48, 216, 4, 6, 6, 0): (_P3, _P3),
              (1, 24, 54, 2, 9, 7, 1): (_P3, _P3), (1, 54, 24, 2, 9, 7, 1): (_P3, _P3),                    # *
              (2, 96, 216, 4, 12, 12, 0): (_P6, _P7),                                                      # *
              (2, 216, 96, 4, 12, 12, 1): (_P6, _P7), (2, 432, 192, 2, 6, 6, 1): (_P6, _P7), (2, 192, 432, 2, 6, 6, 0): (_P6, _P7),
              (2, 54, 54, 2, 8, 8, 1): (_S, _P3),
              (1, 96, 216, 2, 7, 7, 0): (_P3, _P3), (1, 216, 96, 2, 7, 7, 1): (_P3, _P3)}                  # *


def _pw_device_mx(c, dev):
    d = _pw_device(c, dev)
    d.update({k + "_bf": _to_bf(getattr(c, k), dev) for k in ("x", "g", "a")})
    return d


def _pw_forward_mx(ops, c, r, d, what):
    wp = ops.pw_pack(d["w"])
    for xb, yb in ((True, False), (False, True), (True, True)):
        y, partial = ops.pw_fwd(d["x_bf"] if xb else d["x"], d["w"], pre=d["pre"], pre_act=c.act, wp=wp,
                                out_dtype=BF if yb else torch.float32)
        tag = "%s pw_fwd(x %s, y %s)" % (what, "bf16" if xb else "fp32", "bf16" if yb else "fp32")
        if yb:
            _eq_bf(y, r["y"], tag + " y")
            _eq_stats(partial, r["y_st_s0"], r["y_st_s1"], tag + " statistics of the stored y")
        else:
            _eq(y, r["y"], tag + " y")
            _eq_stats(partial, r["sy"], r["sy2"], tag + " statistics")


def _pw_backward_mx(ops, c, r, d, what):
    """Returns the kernel the data gradient (g, a bf16) ran on."""
    from x3dhip import _lib
    N, Ci, Co = c.shape[:3]
    cb, w, pre = d["cb"], d["w"], d["pre"]
    for ga, xb in ((True, False), (False, True), (True, True)):
        g, a, x = d["g_bf" if ga else "g"], d["a_bf" if ga else "a"], d["x_bf" if xb else "x"]
        tag = "%s pw_bwd_weight(g, a %s, x %s)" % (what, "bf16" if ga else "fp32", "bf16" if xb else "fp32")
        _eq(ops.pw_bwd_weight(g, a, cb, x, (Co, Ci), pre=pre, pre_act=c.act), r["dw"], tag)
        df = ops.DeferredGrads()
        dw = ops.pw_bwd_weight(g, a, cb, x, (Co, Ci), pre=pre, pre_act=c.act, defer=df)
        df.flush()
        _eq(dw, r["dw"], tag + " through DeferredGrads")
    wpt = ops.pw_pack(w, transposed=True)
    g, a = d["g_bf"], d["a_bf"]                                           # GA: fp32 outputs, the fp32 case's references
    tag = what + " (g, a bf16)"
    out, partial = ops.pw_bwd_data(g, a, cb, w, x=d["x"] if c.act else None, pre=pre, pre_act=c.act, addend=d["addend"], wpt=wpt)
    kernel = _lib.last_kernel()
    _eq(out, r["dx_add"], tag + " pw_bwd_data + addend%s" % (" + ReLU backward" if c.act else ""))
    if c.act:
        _eq_stats(partial, r["dx_sg"], r["dx_sgx"], tag + " pw_bwd_data statistics")
    out, _ = ops.pw_bwd_data(g, a, cb, w, addend=d["add2"], addend_stride=2, wpt=wpt)
    _eq(out, r["dx_add2"], tag + " pw_bwd_data + stride-2 addend")
    for name, add, astride in (("res0", None, 1), ("res1", d["addend"], 1), ("res2", d["add2"], 2)):
        out, partial = ops.pw_bwd_data_res(g, a, cb, w, d["res_out"], d["res_raw"], addend=add, addend_stride=astride, wpt=wpt)
        _eq(out, r[name], tag + " pw_bwd_data_res " + name)
        _eq_stats(partial, r[name + "_sg"], r[name + "_sgx"], tag + " pw_bwd_data_res statistics " + name)
    if c.act:                                                             # X | Y, and all three flags: x and its gradient bf16
        for ga in (False, True):
            tag = "%s pw_bwd_data(g, a %s, x bf16, out bf16) ReLU backward" % (what, "bf16" if ga else "fp32")
            out, partial = ops.pw_bwd_data(d["g_bf" if ga else "g"], d["a_bf" if ga else "a"], cb, w, x=d["x_bf"], pre=pre,
                                           pre_act=1, wpt=wpt, out_dtype=BF)
            _eq_bf(out, r["dx_act"], tag)
            _eq_stats(partial, r["dx_act_st_s0"], r["dx_act_st_s1"], tag + " statistics of the stored gradient")
    return kernel


@pytest.mark.parametrize("case", ei.PW_MX)
def test_pw_exact_mx(case):
    """Every pointwise entry point but the fused one in the mixed-storage mode, on every kernel that mode has of its own:
    bf16 outputs bitwise RNE of the fp64 reference, their statistics bitwise the fp64 sums over the stored tensor, fp32
    outputs bitwise the fp64 reference."""
    from x3dhip import _lib, ops
    dev = _dev()
    c = ei.pw_mx_case(case)
    r = ei.pw_mx_ref(c)
    d = _pw_device_mx(c, dev)
    _pw_forward_mx(ops, c, r, d, "%s" % (case,))
    kernels = [_lib.last_kernel()]
    for opts in MX_BWD_OPTS:
        with _lib.options(**opts):
            kernels.append(_pw_backward_mx(ops, c, r, d, "%s %s" % (case, opts)))
    assert tuple(kernels) == MX_KERNELS[case] + MX_KERNELS[case][1:], (case, kernels)


@pytest.mark.parametrize("case", ei.PW_MX[:2])
def test_pw_exact_mx_float4_form(case):
    """pw_nt4_min = 0 + no_pwfs: the float4 form of the mixed-storage pw3_kernel (four bf16 values per load / store), which
    under defaults needs 256 workgroups of 256 voxels.  P = 1024 is four full tiles per sample; 24 -> 54 has M blocks of four
    tiles forward and two backward, 54 -> 24 the other way round.  Same inputs and references as test_pw_exact_mx."""
    from x3dhip import _lib, ops
    dev = _dev()
    c = ei.pw_mx_case(case)
    r = ei.pw_mx_ref(c)
    d = _pw_device_mx(c, dev)
    N, Ci, Co = c.shape[:3]
    L = _lib.lib()
    with _lib.options(pw_nt4_min=0, no_pwfs=1):
        assert L.x3d_pw_tiles(N, Ci, Co, 1024, 1) == L.x3d_pw_tiles(N, Co, Ci, 1024, 1) == 4
        _pw_forward_mx(ops, c, r, d, "%s pw_nt4_min 0" % (case,))
        assert _lib.last_kernel() == "pw3_kernel", _lib.last_kernel()
        assert _pw_backward_mx(ops, c, r, d, "%s pw_nt4_min 0" % (case,)) == "pw3_kernel"


def _fused_xy(ops, case, dev, what=""):
    """X3D_MX_X | X3D_MX_Y: x and dx bf16, activation-backward mode without addend."""
    N, Ci, Co, T, H, W, act = case
    assert ops.pw_bwd_fused_ok(Ci, Co, T * H * W, 1, False, ops.MX_X | ops.MX_Y)
    c = ei.fused_mx_case(case)
    r = ei.fused_mx_ref(c)
    g, a, cb, w, pre = (_to(getattr(c, k), dev) for k in ("g", "a", "cb", "w", "pre"))
    tag = "%s %s pw_bwd_fused (x, dx bf16)" % (case, what)
    dx, partial, dw = ops.pw_bwd_fused(g, a, cb, (Co, Ci), ops.pw_pack(w, transposed=True), _to_bf(c.x, dev), xpre=pre, xact=1, mode=1)
    _eq_bf(dx, r["m1_dx0"], tag + " dx")
    _eq(dw, r["m1_dw"], tag + " dW")
    _eq_stats(partial, r["m1_dx0_st_s0"], r["m1_dx0_st_s1"], tag + " statistics of the stored gradient")


@pytest.mark.parametrize("terms", [3, 2])
@pytest.mark.parametrize("case", ei.FUSED_MX)
def test_pw_exact_mx_bwd_fused(case, terms):
    """x3d_pw_bwd_fused: g, a bf16 in modes 0 / 1 / 2 with every addend form (fp32 outputs), x and dx bf16 in mode 1."""
    from x3dhip import _lib, ops
    dev = _dev()
    with _lib.options(bwd_terms=terms):
        _fused(ops, case, dev, "terms %d" % terms, ga_bf=True)
        _fused_xy(ops, case, dev, "terms %d" % terms)


@pytest.mark.parametrize("grid", [3, 40])
def test_pw_exact_mx_long_item_loops(grid):
    """The persistent kernels of the mixed mode (streaming forward, fused backward) with 3 / 40 workgroups, as
    test_pw_exact_integers_long_item_loops (the whole-K forward kernel pw8 has no mixed-storage build: pw8_grid is inert)."""
    from x3dhip import _lib, ops
    dev = _dev()
    with _lib.options(pw8_grid=grid, pw8_max_k=224, fb_grid=grid):
        for case in ei.PW_MX_GRID:
            c = ei.pw_mx_case(case)
            _pw_forward_mx(ops, c, ei.pw_mx_ref(c), _pw_device_mx(c, dev), "%s grid %d" % (case, grid))
            assert _lib.last_kernel() == "pw_fwd_stream_kernel", _lib.last_kernel()
        for case in ei.FUSED_MX_GRID:
            _fused(ops, case, dev, "grid %d" % grid, ga_bf=True)
            _fused_xy(ops, case, dev, "grid %d" % grid)


def _dw_device_mx(c, dev):
    d = {k: _to(getattr(c, k), dev) for k in ("x", "w", "pre", "g", "a", "cb")}
    d.update({k + "_bf": _to_bf(getattr(c, k), dev) for k in ("x", "g", "a")})
    return d


@pytest.mark.parametrize("case", ei.DW_MX)
def test_dw333_exact_mx(case):
    """dw333_fwd (x, y bf16) and dw333_bwd (g, a, x, dx bf16): y and dx bitwise RNE of the fp64 reference, both statistics
    bitwise the fp64 sums over the stored tensors, dw bitwise the fp64 reference."""
    from x3dhip import ops
    dev = _dev()
    c = ei.dw_mx_case(case)
    r = ei.dw_mx_ref(c)
    d = _dw_device_mx(c, dev)
    what = "%s" % (case,)
    y, partial = ops.dw333_fwd(d["x_bf"], d["w"], stride=c.s, pre=d["pre"], pre_act=1)
    _eq_bf(y, r["y"], what + " dw333_fwd y")
    _eq_stats(partial, r["y_st_s0"], r["y_st_s1"], what + " dw333_fwd statistics of the stored y")
    out, dw, bp = ops.dw333_bwd(d["g_bf"], d["a_bf"], d["cb"], d["w"], d["x_bf"], stride=c.s, pre=d["pre"], pre_act=1)
    _eq_bf(out, r["dx"], what + " dw333_bwd dx")
    _eq(dw, r["dw"], what + " dw333_bwd dw")
    _eq_stats(bp, r["dx_st_s0"], r["dx_st_s1"], what + " dw333_bwd statistics of the stored gradient")
    # the same hot inputs in fp32 storage: nothing rounds
    _dw(ops, c, r, d, what + " fp32 storage")


@pytest.mark.parametrize("case", ei.DW_MX)
def test_dw333_exact_bn_forms(case):
    """x3d_dw333_fwd_stats and x3d_dw333_bwd_stats (the producer BN's finalize in the kernel's prologue), fp32 and bf16
    storage: coef, save, the running statistics, dgamma and dbeta bitwise what the fp64 finalize gives on dyadic statistics
    (the same in both storage modes), y / dx and their statistics as in test_dw333_exact_mx."""
    from x3dhip import ops
    _dw_bn_forms(ops, case, _dev())


def _dw_bn_forms(ops, case, dev):
    N, C = case[:2]
    for S in ei.dw_bn_splits(case):
        c, b = ei.dw_mx_bn_fwd_case(case, S)
        r = ei.dw_mx_ref(c)
        d = _dw_device_mx(c, dev)
        sp, gamma, beta = _to(b.sp, dev), _to(b.gamma, dev), _to(b.beta, dev)
        for bf in (False, True):
            what = "%s S = %d dw333_fwd_stats (%s)" % (case, S, "bf16" if bf else "fp32")
            rm, rv = _to(b.rm, dev), _to(b.rv, dev)
            y, partial, coef, save = ops.dw333_fwd_stats(d["x_bf" if bf else "x"], d["w"], sp, S, b.count, gamma, beta, rm.view(-1),
                                                         rv.view(-1), stride=c.s, pre_act=1, momentum=b.momentum, eps=b.eps)
            _eq(coef, b.coef, what + " coef")
            _eq(save, b.save, what + " save")
            _eq(rm, b.rm_new, what + " running mean")
            _eq(rv, b.rv_new, what + " running variance")
            if bf:
                _eq_bf(y, r["y"], what + " y")
                _eq_stats(partial, r["y_st_s0"], r["y_st_s1"], what + " statistics of the stored y")
            else:
                _eq(y, r["y"], what + " y")
                _eq_stats(partial, r["sy"], r["sy2"], what + " statistics")
    c, b = ei.dw_mx_bn_bwd_case(case)
    r = ei.dw_mx_ref(c)
    d = _dw_device_mx(c, dev)
    sp, gamma, save = _to(b.sp, dev), _to(b.gamma, dev), _to(b.save, dev)
    for bf in (False, True):
        what = "%s dw333_bwd(bn=...) (%s)" % (case, "bf16" if bf else "fp32")
        dgamma, dbeta = torch.full((C,), _NAN, device=dev), torch.full((C,), _NAN, device=dev)
        g, a, x = (d[k + "_bf" if bf else k] for k in ("g", "a", "x"))
        out, dw, bp = ops.dw333_bwd(g, a, None, d["w"], x, stride=c.s, pre=d["pre"], pre_act=1,
                                    bn=(sp, b.count, gamma, save, dgamma, dbeta))
        _eq(dgamma, b.dgamma, what + " dgamma")
        _eq(dbeta, b.dbeta, what + " dbeta")
        _eq(dw, r["dw"], what + " dw")
        if bf:
            _eq_bf(out, r["dx"], what + " dx")
            _eq_stats(bp, r["dx_st_s0"], r["dx_st_s1"], what + " statistics of the stored gradient")
        else:
            _eq(out, r["dx"], what + " dx")
            _eq_stats(bp, r["sg"], r["sgx"], what + " statistics")
