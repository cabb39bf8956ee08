"""The grouped update of libx3dstep on the host: x3dstep_apply_groups_host (the code of the kernel through step_core.h)
against the numpy restatement tests/group_ref.py, byte for byte and inside guard bands, with every tensor at its own pair
of scales; the restatement itself against torch.optim.SGD in fp64; the identity with x3dstep_apply_host; the decision; the
refusals; the ABI; the same lists in a sanitised stand-alone program.  No GPU."""
import os
import re
import struct
import subprocess

import numpy as np
import pytest
import torch

from tests import group_cases as grc
from tests import group_ref, guard_ref, step_ref
from tests import guard_cases as gc
from tests import step_program
from x3dhip import _steplib, stepops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = grc.N
F32 = np.float32


def _lib():
    if not os.path.exists(_steplib.LIB_PATH):
        import __graft_entry__ as ge
        ge.build()
    return _steplib.lib()


def _bytes_equal(a, b):
    return np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


def _scales_per_element(hy, off, lr, wd):
    lr_s, wd_s = group_ref.tensor_rule(lr, wd, hy["lr_scale"], hy["wd_scale"])
    return group_ref.per_element(lr_s, off), group_ref.per_element(wd_s, off)


# -- ABI --------------------------------------------------------------------------------------------------------------------
def test_group_header_ctypes_table_and_exports_agree():
    h = _lib()
    src = open(os.path.join(ROOT, "include", "x3dstep.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    funcs = sorted(set(re.findall(r"\b(x3dstep_[a-z0-9_]+)\s*\(", code)))
    assert funcs == sorted(_steplib.SIGNATURES.keys())
    nm = subprocess.run(["nm", "-D", "--defined-only", _steplib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exports = set(re.findall(r" T (x3dstep_[a-z0-9_]+)\n", nm))
    for name in ("x3dstep_hyper_bytes", "x3dstep_apply_groups", "x3dstep_apply_groups_host"):
        assert name in funcs and name in exports
        decl = re.search(r"\b%s\s*\(([^)]*)\)" % name, code).group(1)
        nargs = 0 if decl.strip() == "void" else len(decl.split(","))
        assert nargs == len(_steplib.SIGNATURES[name][1]), name
    assert len(_steplib.SIGNATURES["x3dstep_apply_groups"][1]) == len(_steplib.SIGNATURES["x3dstep_apply_groups_host"][1]) + 1
    assert h.x3dstep_hyper_bytes() == 8 == _steplib.HYPER_DT.itemsize
    assert re.search(r"typedef struct \{\s*float lr_scale;[^}]*float wd_scale;[^}]*\} X3DStepHyper;", src)
    # what existing callers pin is as it was
    assert h.x3dstep_abi_version() == 1 == _steplib.ABI_VERSION and h.x3dstep_header_bytes() == 40
    assert int(re.search(r"#define X3DSTEP_STATE_WORDS (\d+)", src).group(1)) == 8 == _steplib.STATE_WORDS
    assert int(re.search(r"#define X3DSTEP_ABI_VERSION (\d+)", src).group(1)) == 1
    assert h.x3dstep_item_bytes() == 16 and h.x3dstep_keep_bytes() == 24


# -- the restatement against torch.optim.SGD in fp64 ------------------------------------------------------------------------
class _Params(torch.nn.Module):
    """The synthetic table as a module: one fp64 parameter per tensor, named p0, p1, ..."""

    def __init__(self, w, off):
        super().__init__()
        for s in range(len(off) - 1):
            self.register_parameter("p%d" % s, torch.nn.Parameter(
                torch.from_numpy(np.asarray(w[int(off[s]):int(off[s + 1])], dtype=np.float64).copy())))

    def flat(self):
        return np.concatenate([p.detach().numpy() for _, p in self.named_parameters()])


class _FlatStub:
    """What HyperTable reads of a trainer.FlatParams."""

    def __init__(self, off):
        self.offsets = [(int(a), int(b - a)) for a, b in zip(off[:-1], off[1:])]
        self.grad = torch.zeros(1)


def _torch_three_steps(w0, grads, off, hy, lr, wd, mu, coef, gs, nesterov):
    """[(w fp64, m fp64)] after each step of torch.optim.SGD over hypergroups' parameter groups, fed g * coef * gs in fp64
    (exact products here or not, the bound counts their two roundings on the fp32 side)."""
    from x3dhip.hypergroups import HyperTable
    net = _Params(w0, off)
    table = HyperTable(_FlatStub(off), [k for k, _ in net.named_parameters()])
    table.lr_scale[:], table.wd_scale[:] = hy["lr_scale"], hy["wd_scale"]
    groups = table.torch_param_groups(net, lr, wd)
    assert len(groups) == len(set(zip(hy["lr_scale"].tolist(), hy["wd_scale"].tolist())))
    opt = torch.optim.SGD(groups, lr=lr, momentum=float(F32(mu)), nesterov=bool(nesterov))
    out = []
    for g in grads:
        gd = g.astype(np.float64) * float(F32(coef)) * float(F32(gs))
        for s, (_, p) in enumerate(net.named_parameters()):
            p.grad = torch.from_numpy(gd[int(off[s]):int(off[s + 1])].copy())
        opt.step()
        m = np.concatenate([opt.state[p]["momentum_buffer"].numpy() for _, p in net.named_parameters()])
        out.append((net.flat().copy(), m.copy()))
    return out


@pytest.mark.parametrize("nesterov", [0, 1])
@pytest.mark.parametrize("coef,gs", [(1.0, 1.0), (0.5, 0.5), (0.3, 0.125)])
def test_the_restatement_follows_torch_sgd_in_fp64_within_the_counted_roundings(nesterov, coef, gs):
    """Three steps (the first with first = 1) of the restatement in fp32 and of torch.optim.SGD in fp64 with
    torch_param_groups, from the same fp32 start, on the synthetic table with every tensor at its own scales.  The bound
    is group_ref.TorchBound: per step 7 roundings of 2^-24 relative to |w| + lr_s U for w' and 4 relative to M for m'
    (U, M: the sums of the absolute values of the terms of the update and of the momentum), plus the errors of the step's
    inputs carried through the step's linear map.  Nothing in it is fitted."""
    off = gc.synthetic()
    hy = grc.scales(len(off) - 1)
    lr, wd, mu = 0.05, 5e-5, 0.9
    lr_e, wd_e = _scales_per_element(hy, off, lr, wd)
    w0, grads = gc.normals(N, 301), [gc.normals(N, 302 + k) for k in range(3)]
    ref = _torch_three_steps(w0, grads, off, hy, lr, wd, mu, coef, gs, nesterov)
    w, m = w0.copy(), np.zeros(N, F32)
    w64, m64 = w0.astype(np.float64), np.zeros(N)
    bound = group_ref.TorchBound(N)
    for k, g in enumerate(grads):
        bw, bm = bound.step(w64, g, m64, coef, lr_e, wd_e, mu, gs, k == 0, nesterov)
        w, m = group_ref.group_rule(w, g, m, coef, lr_e, wd_e, mu, gs, k == 0, nesterov)
        w64, m64 = ref[k]
        ew, em = np.abs(w.astype(np.float64) - w64), np.abs(m.astype(np.float64) - m64)
        print("step %d nesterov %d: max err w %.3g (bound %.3g at it), m %.3g (bound %.3g)"
              % (k, nesterov, ew.max(), bw[ew.argmax()], em.max(), bm[em.argmax()]))
        assert np.all(ew <= bw) and np.all(em <= bm)


@pytest.mark.parametrize("nesterov", [0, 1])
def test_on_dyadic_inputs_the_restatement_is_torch_sgd_exactly(nesterov):
    """Integers times powers of two, small enough that every operation of three steps is exact in fp32: shown first by
    evaluating the rule in fp64 (where it is exact with room to spare) and comparing, then equal to torch's fp64 result."""
    off = gc.synthetic()
    S = len(off) - 1
    hy = np.zeros(S, dtype=_steplib.HYPER_DT)
    hy["lr_scale"] = [(1.0, 0.0, 0.5, 2.0, 1.0)[s % 5] for s in range(S)]
    hy["wd_scale"] = [(1.0, 0.0, 2.0)[s % 3] for s in range(S)]
    # lr_s >= 2^-2, wd_s >= 2^-1, momentum 2^-1: a step adds at most four fractional bits to w, twelve after three steps
    lr, wd, mu, coef, gs = 0.5, 0.5, 0.5, 0.5, 0.5
    rng = np.random.default_rng(311)
    w0 = rng.integers(-8, 9, N).astype(F32)
    grads = [(rng.integers(-8, 9, N) * 4).astype(F32) for _ in range(3)]
    lr_e, wd_e = _scales_per_element(hy, off, lr, wd)
    ref = _torch_three_steps(w0, grads, off, hy, lr, wd, mu, coef, gs, nesterov)
    w, m = w0.copy(), np.zeros(N, F32)
    w64, m64 = w0.astype(np.float64), np.zeros(N)
    for k, g in enumerate(grads):
        w, m = group_ref.group_rule(w, g, m, coef, lr_e, wd_e, mu, gs, k == 0, nesterov)
        gg = wd_e.astype(np.float64) * w64 + g.astype(np.float64) * coef * gs
        m64 = gg if k == 0 else mu * m64 + gg
        u = mu * m64 + gg if nesterov else m64
        w64 = w64 - lr_e.astype(np.float64) * u
        assert np.array_equal(w.astype(np.float64), w64) and np.array_equal(m.astype(np.float64), m64), "not exact in fp32"
        assert np.array_equal(w64, ref[k][0]) and np.array_equal(m64, ref[k][1])
    assert not np.array_equal(w, w0)


# -- the twin against the restatement ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("shifts", grc.SHIFTS, ids=lambda s: "shift%d%d%d" % s)
def test_groups_twin_equals_the_restatement(shifts):
    _lib()
    off = gc.synthetic()
    w0, m0 = gc.normals(N, 6), gc.normals(N, 7, 0.1)
    for a in grc.GRID:
        h = grc.HostGroup(off, shifts=shifts)
        g, max_norm = grc.gradient_for(a, N, 5)
        h.load(w0, g, m0)
        state0 = h.state.copy()
        h.run(a, g, max_norm)
        coef = h.coef() if a["state"] else F32(1.0)
        assert coef == (F32(0.5) if a["clipped"] else F32(1.0))
        lr_e, wd_e = _scales_per_element(h.hyper, off, gc.LR, a["wd"])
        w1, m1 = group_ref.group_rule(w0, g, m0, coef, lr_e, wd_e, a["mu"], a["gs"], a["first"], a["nesterov"])
        cid = grc.case_id(a)
        assert _bytes_equal(h.w, w1) and _bytes_equal(h.m, m1), cid
        assert _bytes_equal(h.g, g) and h.guards_intact(), cid
        if a["state"]:
            assert h.words() == (0, 0, 0) and int(h.state[_steplib.S_STEP]) == 1
        else:
            assert _bytes_equal(h.state, state0), "no state word is written without a state"
    # the scales show: a tensor at lr_scale 0 keeps w and moves m, and the others move
    s0 = slice(int(off[1]), int(off[2]))
    assert _bytes_equal(h.w[s0], w0[s0]) and not _bytes_equal(h.m[s0], m0[s0]) and not _bytes_equal(h.w, w0)


@pytest.mark.parametrize("n", step_ref.EDGE_LENGTHS)
def test_groups_twin_on_every_edge_length(n):
    """Three tensors (n, 5, n) as the whole buffer at every alignment: an item's head, groups and tail of every size, and a
    neighbour with other scales on both sides."""
    _lib()
    a = dict(first=0, gs=1.0, wd=5e-5, mu=0.9, nesterov=1)
    off = step_ref.seg_off_of([n, 5, n])
    for shifts in grc.SHIFTS:
        h = grc.HostGroup(off, shifts=shifts)
        k = h.t.n
        g, w0, m0 = gc.normals(k, 25), gc.normals(k, 26), gc.normals(k, 27, 0.1)
        h.load(w0, g, m0)
        h.apply_groups(a, state=False)
        lr_e, wd_e = _scales_per_element(h.hyper, off, gc.LR, a["wd"])
        w1, m1 = group_ref.group_rule(w0, g, m0, 1.0, lr_e, wd_e, a["mu"], a["gs"], 0, 1)
        assert _bytes_equal(h.w, w1) and _bytes_equal(h.m, m1) and _bytes_equal(h.g, g) and h.guards_intact()


# -- identity ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("a", gc.ARITH, ids=gc.arith_id)
def test_all_ones_without_nesterov_is_apply_host(a):
    _lib()
    off = gc.synthetic()
    g, max_norm = gc.gradient_for(a, N, 5)
    w0, m0 = gc.normals(N, 6), gc.normals(N, 7, 0.1)
    old, new = gc.HostGuard(off), grc.HostGroup(off, hyper=grc.ones(len(off) - 1))
    for h in (old, new):
        h.load(w0, g, m0)
        h.measure(max_norm)
    old.apply(a)
    new.apply_groups(a)
    assert _bytes_equal(new.w, old.w) and _bytes_equal(new.m, old.m) and _bytes_equal(new.state, old.state)
    assert not _bytes_equal(new.w, w0)
    if not a["clipped"]:
        # the unguarded form is the state form after a clean measure at max_norm = 0
        free = grc.HostGroup(off, hyper=grc.ones(len(off) - 1))
        free.load(w0, g, m0)
        free.apply_groups(a, state=False)
        assert _bytes_equal(free.w, new.w) and _bytes_equal(free.m, new.m)
        assert _bytes_equal(free.state, stepops.new_state())


# -- the decision -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("value", [np.nan, np.inf, -np.inf], ids=["nan", "+inf", "-inf"])
def test_a_planted_nonfinite_leaves_w_and_m_or_is_applied_without_a_state(value):
    _lib()
    off = gc.synthetic()
    a = dict(first=0, gs=1.0, wd=5e-5, mu=0.9, nesterov=1)
    for shifts, at in (((0, 0, 0), 0), ((1, 1, 1), N - 1), ((0, 1, 2), 7000)):
        g, w0, m0 = gc.normals(N, 35), gc.normals(N, 36), gc.normals(N, 37, 0.1)
        g[at] = value
        h = grc.HostGroup(off, shifts=shifts)
        h.load(w0, g, m0)
        h.measure(1.0)
        h.apply_groups(a)
        assert _bytes_equal(h.w, w0) and _bytes_equal(h.m, m0) and _bytes_equal(h.g, g) and h.guards_intact()
        assert h.words() == (1, 1, 1)
        # without a state the same gradient is applied as the arithmetic gives, and no word is written
        f = grc.HostGroup(off, shifts=shifts)
        f.load(w0, g, m0)
        f.apply_groups(a, state=False)
        lr_e, wd_e = _scales_per_element(f.hyper, off, gc.LR, a["wd"])
        w1, m1 = group_ref.group_rule_nonfinite(w0, g, m0, lr_e, wd_e, a["mu"], a["gs"], 0, 1)
        assert group_ref.same_floats(f.w, w1) and group_ref.same_floats(f.m, m1)
        assert not np.isfinite(f.m[at]) and np.all(np.isfinite(np.delete(f.w, at)))
        assert _bytes_equal(f.state, stepops.new_state()) and _bytes_equal(f.g, g) and f.guards_intact()


def test_counters_over_good_bad_bad_good_equal_apply_hosts():
    _lib()
    off = gc.synthetic()
    a = dict(first=0, gs=1.0, wd=5e-5, mu=0.9, nesterov=0)
    old, new = gc.HostGuard(off, R=2), grc.HostGroup(off, R=2)
    good, bad = gc.normals(N, 45), gc.normals(N, 46)
    bad[1234] = np.nan
    w, m = gc.normals(N, 47), gc.normals(N, 48, 0.1)
    old.load(w, None, m)
    new.load(w, None, m)
    seen = []
    for g in (good, bad, bad, good):
        before = (new.w.copy(), new.m.copy())
        old.step(g, a, max_norm=1.0)
        new.load(g=g)
        new.measure(1.0)
        new.apply_groups(a)
        assert new.words() == old.words() and _bytes_equal(new.state, old.state) and _bytes_equal(new.ring, old.ring)
        seen.append(new.words())
        if guard_ref.skips(g):
            assert _bytes_equal(new.w, before[0]) and _bytes_equal(new.m, before[1])
        else:
            assert not _bytes_equal(new.w, before[0])
    assert seen == [(0, 0, 0), (1, 1, 1), (1, 2, 2), (0, 2, 0)]


# -- refusals ---------------------------------------------------------------------------------------------------------------
def _raw_args(h, **kw):
    P = lambda x: x.ctypes.data                          # noqa: E731
    return [kw.get("w", P(h.w)), kw.get("g", P(h.g)), kw.get("m", P(h.m)), kw.get("n", h.t.n),
            kw.get("items", P(h.t.items)), kw.get("nitems", h.t.nitems), kw.get("hyper", P(h.hyper)), kw.get("S", h.t.S),
            kw.get("state", P(h.state)), kw.get("ring", P(h.ring)), kw.get("R", h.R), 0.05, kw.get("mu", 0.9), 5e-5, 1.0,
            kw.get("first", 0), kw.get("nesterov", 0)]


def test_apply_groups_refuses_what_it_cannot_run():
    L = _lib()
    h = grc.HostGroup(step_ref.seg_off_of([5, 70, 2049]))
    n = h.t.n
    h.load(gc.normals(n, 1), gc.normals(n, 2), gc.normals(n, 3))
    before = (h.wbig.copy(), h.mbig.copy(), h.gbig.copy())
    assert L.x3dstep_apply_groups_host(*_raw_args(h)) == -1                 # the step counter is 0
    assert b"nothing has been measured" in L.x3dstep_last_error()
    h.measure()
    state1 = h.state.copy()
    P = lambda x: x.ctypes.data                          # noqa: E731
    gap = h.t.items.copy()
    gap["start"][1] += 1
    short = h.t.items.copy()
    short["len"][-1] -= 1
    swapped = h.t.items.copy()
    swapped[[0, 1]] = swapped[[1, 0]]
    bad = [dict(w=0), dict(g=0), dict(m=0), dict(items=0), dict(hyper=0), dict(ring=0), dict(n=0), dict(n=-1), dict(R=0),
           dict(S=0), dict(nitems=0), dict(w=P(h.w) + 2), dict(g=P(h.g) + 1), dict(hyper=P(h.hyper) + 2),
           dict(state=P(h.state) + 4), dict(m=P(h.w)), dict(m=P(h.w) + 4 * (n - 1)), dict(g=P(h.m) + 8),
           dict(items=P(gap)), dict(items=P(short)), dict(items=P(swapped)), dict(nitems=h.t.nitems - 1), dict(n=n + 1),
           dict(S=2), dict(first=2), dict(first=-1), dict(nesterov=2), dict(nesterov=-1), dict(nesterov=1, mu=0.0),
           dict(nesterov=1, mu=-0.5)]
    for field, value in (("lr_scale", -1.0), ("lr_scale", np.nan), ("wd_scale", np.inf), ("wd_scale", -np.inf)):
        hy = h.hyper.copy()
        hy[field][1] = value
        bad.append(dict(hyper=P(hy), _keep=hy))
    for kw in bad:
        assert L.x3dstep_apply_groups_host(*_raw_args(h, **kw)) == -1, list(kw)
        assert L.x3dstep_last_error() and b"x3dstep_apply_groups_host" in L.x3dstep_last_error()
    assert _bytes_equal(h.wbig, before[0]) and _bytes_equal(h.mbig, before[1]) and _bytes_equal(h.gbig, before[2])
    assert _bytes_equal(h.state, state1), "a refused call writes nothing"
    # the unguarded form needs neither state nor ring
    assert L.x3dstep_apply_groups_host(*_raw_args(h, state=0, ring=0, R=0)) == 0
    assert _bytes_equal(h.state, state1) and not _bytes_equal(h.wbig, before[0])
    assert L.x3dstep_apply_groups_host(*_raw_args(h)) == 0
    with pytest.raises(ValueError):
        stepops.apply_groups_host(h.w, h.g, h.m, h.t, h.hyper[:-1], None, None, 0, 0.1)
    with pytest.raises(ValueError):
        stepops.apply_groups_host(h.w, h.g, h.m, h.t, h.hyper, None, None, 0, 0.1, momentum=0.0, nesterov=True)
    with pytest.raises(ValueError):
        stepops.apply_groups_host(h.w[:-1], h.g, h.m, h.t, h.hyper, None, None, 0, 0.1)


def test_the_twin_refuses_every_item_the_kernel_would_leave_out():
    """One bad item of each kind (tests/group_cases.py): the twin, whose tables are host memory, refuses the call and
    writes nothing.  That exactly that item is left untouched is shown on the per-item code itself by
    tests/group_check.cpp (below) and on the kernel by tests/test_group_gpu.py."""
    L = _lib()
    h = grc.HostGroup(gc.synthetic())
    h.load(gc.normals(N, 1), gc.normals(N, 2), gc.normals(N, 3))
    before = (h.wbig.copy(), h.mbig.copy())
    cases = grc.bad_item_tables(h.t)
    assert len(cases) == 10
    for name, items, hy, _ in cases:
        rc = L.x3dstep_apply_groups_host(*_raw_args(h, items=items.ctypes.data, hyper=hy.ctypes.data, state=0, ring=0, R=0))
        assert rc == -1 and L.x3dstep_last_error(), name
    assert _bytes_equal(h.wbig, before[0]) and _bytes_equal(h.mbig, before[1])


# -- the same lists under the sanitisers ------------------------------------------------------------------------------------
def _write_case(f, off, R, shifts, hy, steps, seed):
    """One case of tests/group_check.cpp's file, with what the in-process twin gave as the expectation."""
    h = grc.HostGroup(off, hyper=hy, R=R, shifts=shifts)
    n = h.t.n
    w0, m0 = gc.normals(n, seed), gc.normals(n, seed + 1, 0.1)
    h.load(w0, None, m0)
    f.write(struct.pack("<IIIIII", h.t.S, R, len(steps), *shifts))
    f.write(np.asarray(off, "<i8").tobytes())
    f.write(hy.tobytes())
    f.write(w0.astype("<f4").tobytes() + m0.astype("<f4").tobytes())
    for g, max_norm, a in steps:
        h.run(a, g, max_norm)
        f.write(struct.pack("<dffffIII", max_norm, gc.LR, a["mu"], a["wd"], a["gs"], a["first"], a["nesterov"],
                            1 if a["state"] else 0))
        f.write(g.astype("<f4").tobytes() + h.w.astype("<f4").tobytes() + h.m.astype("<f4").tobytes())
    f.write(h.state.astype("<i8").tobytes())


def test_the_same_lists_in_a_sanitised_stand_alone_program(tmp_path):
    """step_host.cpp and step_core.h compiled with -fsanitize=address,undefined into a program of their own
    (tests/group_check.cpp), built and run as tests/guard_check.cpp is: a child process, every buffer a heap block of
    exactly the size the library is told; nothing sanitised is loaded into this interpreter.  The program also runs the
    kernel's per-item walk (group_resolve, group_lane) over the tables with one bad item each and checks that exactly that
    item is untouched."""
    step_program.compiler()
    _lib()
    syn = gc.synthetic()
    S = len(syn) - 1
    good, bad = gc.normals(N, 91), gc.normals(N, 92)
    bad[int(syn[9]) + 7] = np.nan
    base = dict(first=0, nesterov=1, mu=0.9, gs=0.5, wd=5e-5, state=True, clipped=False)
    free = dict(base, state=False)
    cases = [(syn, 2, (0, 0, 0), grc.scales(S), [(good, 0.0, dict(base, first=1)), (bad, 1.0, base), (good, 10.0, base),
                                                 (good, 0.0, free)], 400),
             (syn, 3, (1, 1, 1), grc.scales(S), [(gc.eights(N, 93), 512.0, dict(base, nesterov=0)), (good, 0.0, free)], 410),
             (syn, 3, (3, 3, 3), grc.ones(S), [(good, 10.0, dict(base, nesterov=0, mu=0.0))], 420),
             (syn, 3, (0, 1, 2), grc.scales(S), [(good, 10.0, base), (good, 0.0, free)], 430)]
    for n in step_ref.EDGE_LENGTHS:
        off = step_ref.seg_off_of([n, 5, n])
        cases.append((off, 1, (n % 4,) * 3, grc.scales(3), [(gc.normals(2 * n + 5, 94), 0.5, base)], 440 + n))
    path = str(tmp_path / "group_cases.bin")
    with open(path, "wb") as f:
        f.write(struct.pack("<I", len(cases)))
        for c in cases:
            _write_case(f, *c)
    last, out = step_program.run(tmp_path, "group_check", path)
    assert last[:2] == ["groups", str(len(cases))] and last[2] == "items" and int(last[3]) == 10, out[-500:]
    assert int(last[-1]) == 0, out[-500:]
