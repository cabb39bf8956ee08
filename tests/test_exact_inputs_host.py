"""The proof behind tests/test_exact_gpu.py, on the CPU: on the inputs of tests/exact_inputs.py every op, evaluated in
torch fp32 in two different summation orders and in fp64, gives bitwise the same result, and the any-order exactness
condition sum |terms| / u < 2^24 holds for every output kind of every case the GPU tests use.  For the split-term probes
the bf16 split is emulated: the six products the kernels keep reproduce the fp64 result exactly, leaving out any one a
probe kind is there for changes at least 3 of 4 outputs in every 16-row x 32-voxel tile, and the two-term form cannot
reproduce the probes that carry a lo term.  For the mixed-storage cases (hot integer inputs) additionally: every bf16
operand is a bf16 tensor, the bf16 stores round often enough and in every way (ties and non-ties, up and down), and three wrong
stores / statistics computed from the references alone differ from them.  So a mismatch on the GPU is the kernel's fault."""
import math

import pytest
import torch

from tests import exact_inputs as ei
from tests.exact_inputs import DW_ALL, FUSED_ALL, HEAD_EXACT, PW_ALL, STEM_EXACT


def _three_ways(ref, mags, case, what):
    r64 = ref(case, torch.float64, 0)
    ei.assert_exact(mags(case, r64), what)
    for order in (0, 1):
        r32 = ref(case, torch.float32, order)
        assert set(r32) == set(r64)
        for k, v in r32.items():
            assert v.dtype == torch.float32
            assert torch.equal(v.double(), r64[k]), "%s %s: fp32 (order %d) differs from fp64" % (what, k, order)
    r64b = ref(case, torch.float64, 1)
    for k, v in r64b.items():
        assert torch.equal(v, r64[k]), "%s %s: the two evaluation orders disagree in fp64" % (what, k)


def test_unit_of_and_the_exactness_condition():
    assert ei.unit_of(torch.tensor([0.5, 3.0, 0.75])) == 0.25
    assert ei.unit_of(torch.tensor([4.0, -8.0])) == 4.0
    assert ei.unit_of(torch.zeros(3)) == 1.0
    assert ei.unit_of(torch.tensor([ei.PROBE_V], dtype=torch.float64)) == 2.0 ** -20
    ei.assert_exact({"ok": (torch.tensor([2.0 ** 24 - 1]), 1.0)})
    with pytest.raises(AssertionError):
        ei.assert_exact({"too long a sum": (torch.tensor([2.0 ** 22]), 0.25)})
    # the condition is not decoration: 2^24 + 1 is the first integer fp32 cannot hold
    assert float(torch.tensor(2.0 ** 24) + torch.tensor(1.0)) == 2.0 ** 24


def test_sparse_rows_hit_every_column_and_tap():
    for M, K, nnz in [(54, 24, 4), (24, 54, 4), (192, 432, 4), (432, 96, 4), (2, 27, 3), (3, 27, 3), (24, 27, 4), (24, 5, 2)]:
        w = ei.sparse_rows(M, K, nnz, 5)
        assert bool((w != 0).any(0).all()) and set(w.unique().tolist()) <= {0.0, 0.5, -0.5, 1.0, -1.0}
        assert int((w != 0).sum(1).max()) == max(nnz, -(-K // M))


@pytest.mark.parametrize("case", PW_ALL)
def test_pw_integer_cases_are_exact_in_any_order(case):
    c = ei.pw_case(case)
    xin = ei.affine(c.pre, c.x) if c.act else c.x
    assert set(xin.unique().tolist()) <= {0.0, 1.0, -1.0, 2.0, -2.0}              # the effective activations
    _three_ways(ei.pw_ref, ei.pw_mags, c, "pw %s" % (case,))


@pytest.mark.parametrize("case", FUSED_ALL)
def test_pw_fused_integer_cases_are_exact_in_any_order(case):
    _three_ways(ei.fused_ref, ei.fused_mags, ei.fused_case(case), "fused %s" % (case,))


@pytest.mark.parametrize("case", DW_ALL)
def test_dw333_integer_cases_are_exact_in_any_order(case):
    c = ei.dw_case(case)
    assert bool((c.w.view(case[1], 27) != 0).any(0).all())                          # all 27 taps
    _three_ways(ei.dw_ref, ei.dw_mags, c, "dw333 %s" % (case,))


@pytest.mark.parametrize("shape", STEM_EXACT)
def test_stem_integer_cases_are_exact_in_any_order(shape):
    _three_ways(ei.stem_ref, ei.stem_mags, ei.stem_case(shape), "stem %s" % (shape,))


@pytest.mark.parametrize("R", ei.HEAD_R)
def test_head_integer_cases_are_exact_in_any_order(R):
    for (r, K, J, C) in HEAD_EXACT:
        if r == R:
            _three_ways(ei.head_ref, ei.head_mags, ei.head_case(R, K, J, C), "head %s" % ((R, K, J, C),))


# --------------------------------------------------------------------------------------------------------- probes
def test_probe_values_split_into_three_nonzero_terms():
    s = ei.split3(torch.tensor([ei.PROBE_V, -ei.PROBE_V, ei.PROBE_B, 1.0, 0.0], dtype=torch.float64))
    assert s["hi"].tolist() == [1.0, -1.0, 1.0, 1.0, 0.0]
    assert s["mid"].tolist() == [2.0 ** -10, -2.0 ** -10, 2.0 ** -10, 0.0, 0.0]
    assert s["lo"].tolist() == [2.0 ** -20, -2.0 ** -20, 0.0, 0.0, 0.0]
    assert sorted(set(p for k in ei.PROBE_KINDS for p in ei.NEEDS[k])) == sorted(ei.KEPT)      # every kept product is probed


def _probe_proof(A, B, ref, kind, what):
    """A [M, K], B [K, cols] fp64 probe operands, ref = A B [M, cols]."""
    assert torch.equal(A.float().double(), A) and torch.equal(B.float().double(), B)           # fp32 values
    assert torch.equal(A @ B, ref)
    cnt = ei.probe_count(A, B)
    assert float(cnt.max()) <= 8
    ei.assert_exact({"probe": (A.abs() @ B.abs(), 2.0 ** -20)}, what)
    assert float((A.abs() @ B.abs()).max()) < 16
    # the signed count m of an output is +-(its number of non-zero products): never 0 where a product exists
    m = torch.sign(A) @ torch.sign(B)
    assert torch.equal(m.abs(), cnt)
    # fp32 in two orders
    perm = torch.arange(A.shape[1] - 1, -1, -1)
    for got in (A.float() @ B.float(), A.float()[:, perm] @ B.float()[perm]):
        assert torch.equal(got.double(), ref), what
    sa, sb = ei.split3(A), ei.split3(B)
    prod = {(p, q): sa[p] @ sb[q] for p in ("hi", "mid", "lo") for q in ("hi", "mid", "lo")}
    for pq in (("mid", "lo"), ("lo", "mid"), ("lo", "lo")):                                    # dropped by design: zero here
        assert not bool(prod[pq].any()), (what, pq)
    assert torch.equal(sum(prod[pq] for pq in ei.KEPT), ref), what + ": the six kept products do not reproduce the result"
    for pq in ei.KEPT:
        without = sum(prod[o] for o in ei.KEPT if o != pq)
        if pq in ei.NEEDS[kind]:
            assert not torch.equal(without, ref)
            yield pq, without != ref
        else:
            assert not bool(prod[pq].any()), (what, pq)
    if kind in ei.CARRIES_LO:
        two = prod[("hi", "hi")] + prod[("hi", "mid")] + prod[("mid", "hi")]
        yield "two-term", two != ref


def _resolved(changed, N, what):
    """changed [M, N * P] -> every 16 x 32 tile of every sample: at least 3 of 4 outputs change."""
    M = changed.shape[0]
    frac = ei.tiles_resolved(changed.view(M, N, -1).transpose(0, 1))
    assert frac >= 0.75, "%s: a tile where only %.2f of the outputs resolve the term" % (what, frac)


_FWD_SHAPES = sorted(set(s for v in ei.PROBE_FWD.values() for s in v))


@pytest.mark.parametrize("kind", ei.PROBE_KINDS)
@pytest.mark.parametrize("shape", _FWD_SHAPES)
def test_forward_probes_resolve_every_kept_product(shape, kind):
    N, Ci, Co, T, H, W = shape
    w, x, y = ei.probe_fwd(shape, kind)
    A, B = w, x.flatten(2).transpose(0, 1).reshape(Ci, -1)
    ref = y.flatten(2).transpose(0, 1).reshape(Co, -1)
    for pq, changed in _probe_proof(A, B, ref, kind, "fwd %s %s" % (shape, kind)):
        _resolved(changed, N, "fwd %s %s without %s" % (shape, kind, pq))


@pytest.mark.parametrize("kind", ei.PROBE_KINDS)
@pytest.mark.parametrize("shape", sorted(set(ei.PROBE_DGRAD + ei.PROBE_FUSED)))
def test_data_gradient_probes_resolve_every_kept_product(shape, kind):
    N, Ci, Co, T, H, W = shape
    w, dY, dX = ei.probe_dgrad(shape, kind)
    A, B = w.t(), dY.flatten(2).transpose(0, 1).reshape(Co, -1)
    ref = dX.flatten(2).transpose(0, 1).reshape(Ci, -1)
    for pq, changed in _probe_proof(A, B, ref, kind, "dgrad %s %s" % (shape, kind)):
        _resolved(changed, N, "dgrad %s %s without %s" % (shape, kind, pq))


@pytest.mark.parametrize("kind", ei.PROBE_KINDS)
@pytest.mark.parametrize("shape", sorted(set(ei.PROBE_WGRAD + ei.PROBE_FUSED)))
def test_weight_gradient_probes_resolve_every_kept_product(shape, kind):
    N, Ci, Co, T, H, W = shape
    dY, x, dW = ei.probe_wgrad(shape, kind)
    A = dY.flatten(2).transpose(0, 1).reshape(Co, -1)
    B = x.flatten(2).transpose(0, 1).reshape(Ci, -1).t()
    for pq, changed in _probe_proof(A, B, dW, kind, "wgrad %s %s" % (shape, kind)):
        _resolved(changed, 1, "wgrad %s %s without %s" % (shape, kind, pq))


# --------------------------------------------------------------------------------------------------------- mixed storage
# The proof behind section 5 of tests/test_exact_gpu.py.  Per case: (a) the any-order condition and fp32 in two orders ==
# fp64 for every output, the stored tensors' statistics included; (b) every tensor a kernel reads as bf16 is a bf16 tensor;
# (c) the bf16 stores really round -- ties in both directions, non-ties in both directions, enough of them to move the
# statistics of a quarter of the rows; (d) controls from the references alone: a store by truncation, a store that rounds half
# away from zero and statistics of the unrounded tensor all DIFFER from the reference, so the GPU comparison can fail for each
# of the three mistakes.
MIN_INEXACT, MIN_ROWS = 32, 0.25


def _rounding_is_exercised(r, name, s0, s1, what):
    cen = ei.rounding_census(r[name])
    assert cen["inexact"] >= MIN_INEXACT, "%s %s: only %d outputs are not bf16 numbers" % (what, name, cen["inexact"])
    for k in ("tie_up", "tie_down", "up", "down"):
        assert cen[k] > 0, "%s %s: no rounding of the kind '%s' (%s)" % (what, name, k, cen)
    for k, ref in (("_st_s0", s0), ("_st_s1", s1)):
        moved = float((r[name + k] != r[ref]).double().mean())
        assert moved >= MIN_ROWS, "%s %s: %s differs from the unrounded tensor's in %.2f of the rows only" % (what, name, k, moved)
    return cen


def _controls(r, name, s0, s1, cen, what):
    v, st = r[name], r[name + "_st"]
    trunc, away = ei.stored_by_truncation(v), ei.stored_half_away(v)
    assert bool((trunc.abs() <= v.abs()).all()) and ei.bf16_ok(trunc) and ei.bf16_ok(away)
    # truncation misses exactly what RNE rounds up in magnitude, half-away-from-zero exactly the ties RNE rounds down
    assert int((trunc != st).sum()) == cen["tie_up"] + cen["up"] > 0, what
    assert int((away != st).sum()) == cen["tie_down"] > 0, what
    assert not torch.equal(r[s0], r[name + "_st_s0"]) and not torch.equal(r[s1], r[name + "_st_s1"]), what


def _two_terms_suffice(c, others, what):
    """bwd_terms = 2 keeps hi.hi, hi.mid, mid.hi: exact when one operand of every backward GEMM is pure hi and the other has
    no lo term.  dY (up to 11 bits next to a hot g) is hi + mid; weights and activations are bf16 numbers."""
    s = ei.split3(ei.dy_of(c.cb, c.g, c.a))
    assert not bool(s["lo"].any()), what
    for t in others:
        assert ei.bf16_ok(t), what
    return s["hi"].abs() + s["mid"].abs()                               # sum |terms| of the split dY


def test_bf16_store_models():
    v = torch.tensor([1.0, 128.5, 129.5, -128.5, -129.5, 256.5, 257.5, -257.5, 130.25, 130.75, 0.0], dtype=torch.float64)
    assert ei.stored(v).tolist() == [1.0, 128.0, 130.0, -128.0, -130.0, 256.0, 258.0, -258.0, 130.0, 131.0, 0.0]
    assert ei.stored_by_truncation(v).tolist() == [1.0, 128.0, 129.0, -128.0, -129.0, 256.0, 256.0, -256.0, 130.0, 130.0, 0.0]
    assert ei.stored_half_away(v).tolist() == [1.0, 129.0, 130.0, -129.0, -130.0, 256.0, 258.0, -258.0, 130.0, 131.0, 0.0]
    assert ei.rounding_census(v) == {"inexact": 9, "tie_up": 2, "tie_down": 2, "up": 3, "down": 2}
    assert ei.bf16_ok(torch.tensor([127.5, 255.0, -64.5])) and not ei.bf16_ok(torch.tensor([128.5]))


def test_mx_case_lists_are_rows_of_the_mixed_storage_tables():
    from tests import test_mixed_storage_gpu as mg
    pw_rows = set(tuple(r[:6]) for r in mg.PW_FWD) | set(tuple(r[:6]) for r in mg.PW_BWD)
    assert set(c[:6] for c in ei.PW_MX) <= pw_rows
    assert set(c[:6] for c in ei.FUSED_MX) == set(mg.FUSED)
    assert set(ei.DW_MX) <= set(mg.DW)
    # every row where the mixed mode runs another kernel than fp32
    for row in [(1, 96, 216, 2, 7, 7), (1, 216, 96, 2, 7, 7), (2, 96, 216, 4, 12, 12), (1, 24, 54, 2, 9, 7), (1, 54, 24, 2, 9, 7)]:
        assert row in set(c[:6] for c in ei.PW_MX)
    for row in [(1, 5, 5, 13, 9, 1), (1, 3, 3, 15, 11, 2), (1, 33, 2, 4, 4, 2), (1, 2, 3, 40, 56, 1)]:
        assert row in ei.DW_MX


def _pw_mx_proof(case):
    c = ei.pw_mx_case(case)
    what = "pw mx %s" % (case,)
    for t in (c.x, c.g, c.a):                                           # x after raw_for: what the kernel is handed
        assert ei.bf16_ok(t), what
    _three_ways(ei.pw_mx_ref, ei.pw_mx_mags, c, what)
    r = ei.pw_mx_ref(c)
    xin = torch.relu(ei.affine(c.pre, c.x)) if c.act else c.x
    dym = _two_terms_suffice(c, (c.w, xin), what)
    m = ei.pw_mags(c, r)
    ei.assert_exact({"din, two terms": (ei._pw_dgrad(dym, c.w.abs(), 0), m["din"][1]),
                     "dw, two terms": (ei._pw_wgrad(dym, xin.abs(), 1, 0), m["dw"][1])}, what)
    for name, s0, s1 in [("y", "sy", "sy2")] + ([("dx_act", "dx_act_s0", "dx_act_s1")] if c.act else []):
        _controls(r, name, s0, s1, _rounding_is_exercised(r, name, s0, s1, what), what)


@pytest.mark.parametrize("case", ei.PW_MX + ei.PW_MX_GRID)
def test_pw_mx_cases_are_exact_and_their_bf16_stores_round(case):
    _pw_mx_proof(case)


@pytest.mark.parametrize("case", ei.FUSED_MX + ei.FUSED_MX_GRID)
def test_pw_fused_mx_cases_are_exact_and_their_bf16_stores_round(case):
    c = ei.fused_mx_case(case)
    what = "fused mx %s" % (case,)
    for t in (c.x, c.g, c.a):
        assert ei.bf16_ok(t), what
    _three_ways(ei.fused_mx_ref, ei.fused_mx_mags, c, what)
    r = ei.fused_mx_ref(c)
    xin = torch.relu(ei.affine(c.pre, c.x))
    dym = _two_terms_suffice(c, (c.w, c.x, xin, c.xo), what)
    m = ei.fused_mags(c, r)
    ei.assert_exact({"din, two terms": (ei._pw_dgrad(dym, c.w.abs(), 0), m["m0_dx"][1]),
                     "dw, two terms": (ei._pw_wgrad(dym, torch.maximum(c.x.abs(), c.xo), 1, 0), min(m["m0_dw"][1], m["m2_dw"][1]))}, what)
    _controls(r, "m1_dx0", "m1_dx0_sg", "m1_dx0_sgx", _rounding_is_exercised(r, "m1_dx0", "m1_dx0_sg", "m1_dx0_sgx", what), what)


def _dw_mx_proof(c, outs, what):
    for t in (c.x, c.g, c.a):
        assert ei.bf16_ok(t), what
    _three_ways(ei.dw_mx_ref, ei.dw_mx_mags, c, what)
    r = ei.dw_mx_ref(c)
    for name, s0, s1 in outs:
        _controls(r, name, s0, s1, _rounding_is_exercised(r, name, s0, s1, what), what)


_DW_Y, _DW_DX = ("y", "sy", "sy2"), ("dx", "sg", "sgx")


@pytest.mark.parametrize("case", ei.DW_MX)
def test_dw333_mx_cases_are_exact_and_their_bf16_stores_round(case):
    c = ei.dw_mx_case(case)
    assert bool((c.w.view(case[1], 27) != 0).any(0).all())
    _dw_mx_proof(c, (_DW_Y, _DW_DX), "dw333 mx %s" % (case,))


@pytest.mark.parametrize("case", ei.DW_MX)
def test_dw333_bn_forward_form_is_exact(case):
    """x3d_dw333_fwd_stats: the kernel's fp64 finalize, restated step by step on the case's partials in two summation orders,
    gives the case's coefficients, saved statistics and running statistics without a rounding, all of them fp32 numbers."""
    N, C = case[:2]
    for S in ei.dw_bn_splits(case):
        c, b = ei.dw_mx_bn_fwd_case(case, S)
        what = "dw333 fwd_stats %s S = %d" % (case, S)
        assert torch.equal(b.sp.float().double(), b.sp)
        ns = N // S
        cnt = float(b.count * ns)
        assert math.log2(cnt - 1) % 1 == 0
        for order in (0, 1):
            sp = b.sp.view(ns, S, C, -1, 2).permute(1, 2, 0, 3, 4).reshape(S, C, -1, 2)        # split j: samples j, j + S, ...
            s = (sp.flip(2) if order else sp).sum(2)
            mean = s[..., 0] / cnt
            var = s[..., 1] / cnt - mean * mean
            invstd = 1.0 / torch.sqrt(var + b.eps)
            sc = b.gamma * invstd
            coef = torch.stack([sc, b.beta - mean * b.gamma * invstd], -1)
            assert torch.equal(coef.repeat(ns, 1, 1), b.coef) and torch.equal(torch.stack([mean, invstd]), b.save), what
            assert torch.equal((1.0 - b.momentum) * b.rm + b.momentum * mean, b.rm_new), what
            assert torch.equal((1.0 - b.momentum) * b.rv + b.momentum * (var * cnt / (cnt - 1.0)), b.rv_new), what
            assert bool((var > 0).all())
        for t in (b.coef, b.save, b.rm_new, b.rv_new, b.gamma, b.beta, b.rm, b.rv):
            assert torch.equal(t.float().double(), t), what
        assert torch.equal(c.pre, b.coef)
        _dw_mx_proof(c, (_DW_Y,), what)


@pytest.mark.parametrize("case", ei.DW_MX)
def test_dw333_bn_backward_form_is_exact(case):
    """x3d_dw333_bwd_stats: likewise its backward finalize -- cb, dgamma, dbeta."""
    N, C = case[:2]
    c, b = ei.dw_mx_bn_bwd_case(case)
    what = "dw333 bwd_stats %s" % (case,)
    M = float(b.count * N)
    assert math.log2(M) % 1 == 0 and torch.equal(b.sp.float().double(), b.sp)
    mean, invstd = b.save[0, 0], b.save[1, 0]
    for order in (0, 1):
        sp = b.sp.permute(1, 0, 2, 3).reshape(C, -1, 2)
        s = (sp.flip(1) if order else sp).sum(1)
        sg, sga = s[:, 0], s[:, 1]
        sgx = (sga - mean * sg) * invstd
        k = b.gamma * invstd
        cb = torch.stack([k, -k * invstd * sgx / M, -k * sg / M + k * invstd * mean * sgx / M], -1)
        assert torch.equal(cb[None].repeat(N, 1, 1), b.cb) and torch.equal(sgx, b.dgamma) and torch.equal(sg, b.dbeta), what
    for t in (b.cb, b.dgamma, b.dbeta, b.gamma, b.save):
        assert torch.equal(t.float().double(), t), what
    assert torch.equal(c.cb, b.cb)
    _dw_mx_proof(c, (_DW_DX,), what)


@pytest.mark.parametrize("proof,case", [(_pw_mx_proof, ei.PW_MX[0]), (_pw_mx_proof, ei.PW_MX[5]),
                                        (test_pw_fused_mx_cases_are_exact_and_their_bf16_stores_round, ei.FUSED_MX[0]),
                                        (test_dw333_mx_cases_are_exact_and_their_bf16_stores_round, ei.DW_MX[1]),
                                        (test_dw333_bn_forward_form_is_exact, ei.DW_MX[3]),
                                        (test_dw333_bn_backward_form_is_exact, ei.DW_MX[4])])
def test_a_weakened_hot_pattern_fails_the_rounding_conditions(monkeypatch, proof, case):
    """The conditions are not decoration: with hot values of 8 every output stays below 64 on a grid of 1/4 or coarser, which
    eight bits hold -- the case is still exact, but no bf16 store rounds, and the proof must say so."""
    monkeypatch.setattr(ei, "HOT", (8., -8., 8., -8., 8., -8.))
    with pytest.raises(AssertionError, match="outputs are not bf16 numbers"):
        proof(case)


def test_a_hot_pattern_of_one_magnitude_fails_the_rounding_conditions(monkeypatch):
    """With 128 alone the forward outputs of a conv behind a ReLU round, but every rounding is a tie: a store that is right
    at the midpoint and wrong off it would pass."""
    monkeypatch.setattr(ei, "HOT", (128., -128., 128., -128., 128., -128.))
    with pytest.raises(AssertionError, match="no rounding of the kind"):
        _pw_mx_proof(ei.PW_MX[0])
