"""The trust ratios of libx3dstep on the host: x3dstep_trust_host and x3dstep_apply_lars_host (the code of the kernels
through step_core.h) against the numpy restatement tests/lars_ref.py, byte for byte and inside guard bands, with every
tensor at its own rate of trust and scales; the restatement itself against a LARS in plain torch, fp64; the identities with
x3dstep_measure_host and x3dstep_apply_groups_host; non-finite values; the refusals; the ABI; the same lists in a sanitised
stand-alone program.  No GPU."""
import os
import re
import struct
import subprocess

import numpy as np
import pytest
import torch

from tests import group_cases as grc
from tests import group_ref, lars_ref, step_ref
from tests import guard_cases as gc
from tests import lars_cases as lc
from tests import step_program
from x3dhip import _steplib, stepops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = lc.N
F32 = np.float32


def _lib():
    if not os.path.exists(_steplib.LIB_PATH):
        import __graft_entry__ as ge
        ge.build()
    return _steplib.lib()


def _bytes_equal(a, b):
    return np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


def _per_element(hy, off, lr, wd):
    lr_s, wd_s = group_ref.tensor_rule(lr, wd, hy["lr_scale"], hy["wd_scale"])
    return group_ref.per_element(lr_s, off), group_ref.per_element(wd_s, off)


def _expected_trust(h, a, lr=gc.LR, coef=None):
    """The restatement's trust from the twin's own sums (whose bytes the identity test holds against measure_host)."""
    _, gss, _, nf = h.record()
    coef = h.coef() if coef is None else coef
    return lars_ref.trust_rule(h.wsumsq, gss, nf, h.eta, h.hyper["lr_scale"], h.hyper["wd_scale"], lr, a["wd"], a["gs"], coef,
                               a.get("eps", lc.EPS), a.get("clip", 0))


# -- ABI --------------------------------------------------------------------------------------------------------------------
def test_lars_header_ctypes_table_and_exports_agree():
    h = _lib()
    src = open(os.path.join(ROOT, "include", "x3dstep.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    nm = subprocess.run(["nm", "-D", "--defined-only", _steplib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exports = set(re.findall(r" T (x3dstep_[a-z0-9_]+)\n", nm))
    want = {"x3dstep_trust_workspace_bytes": 1, "x3dstep_trust": 20, "x3dstep_trust_host": 19, "x3dstep_apply_lars": 19,
            "x3dstep_apply_lars_host": 18}
    for name, count in want.items():
        assert name in exports and name in _steplib.SIGNATURES
        decl = re.search(r"\b%s\s*\(([^)]*)\)" % name, code).group(1)
        assert len(decl.split(",")) == count == len(_steplib.SIGNATURES[name][1]), name
    # x3dstep_apply_lars is x3dstep_apply_groups with one more pointer, after hyper
    ag, al = _steplib.SIGNATURES["x3dstep_apply_groups"][1], _steplib.SIGNATURES["x3dstep_apply_lars"][1]
    assert al == ag[:7] + [_steplib._P] + ag[7:]
    assert h.x3dstep_abi_version() == 1 == _steplib.ABI_VERSION
    assert int(re.search(r"#define X3DSTEP_ABI_VERSION (\d+)", src).group(1)) == 1
    assert h.x3dstep_hyper_bytes() == 8 and h.x3dstep_item_bytes() == 16 and h.x3dstep_header_bytes() == 40
    assert h.x3dstep_trust_workspace_bytes(7) == 56 and h.x3dstep_trust_workspace_bytes(0) == 0
    assert stepops.trust_workspace_bytes(2092) == 8 * 2092
    with pytest.raises(ValueError):
        stepops.trust_workspace_bytes(0)


# -- the restatement against a LARS in plain torch, fp64 ----------------------------------------------------------------------
def _torch_lars_three_steps(w0, grads, off, hy, eta, lr, wd, mu, coef, gs, eps, clip, nesterov):
    """[(w fp64, m fp64, r fp64 per element)] after each step of: norms by torch.linalg.vector_norm, p.grad = trust *
    (g + wd_s * w), torch.optim.SGD(weight_decay=0) with the tensor's rate lr_s."""
    S = len(off) - 1
    lr_s, wd_s = group_ref.tensor_rule(lr, wd, hy["lr_scale"], hy["wd_scale"])
    ps = [torch.nn.Parameter(torch.from_numpy(w0[int(off[s]):int(off[s + 1])].astype(np.float64))) for s in range(S)]
    opt = torch.optim.SGD([dict(params=[p], lr=float(lr_s[s])) for s, p in enumerate(ps)], lr=lr, momentum=float(F32(mu)),
                          weight_decay=0.0, nesterov=bool(nesterov))
    out = []
    for g in grads:
        gd = g.astype(np.float64) * float(F32(coef)) * float(F32(gs))
        rs = np.ones(S)
        for s, p in enumerate(ps):
            gt = torch.from_numpy(gd[int(off[s]):int(off[s + 1])].copy())
            a, b = float(torch.linalg.vector_norm(p.detach())), float(torch.linalg.vector_norm(gt))
            r = 1.0
            if float(eta[s]) > 0 and a > 0 and b > 0:
                r = float(eta[s]) * a / (b + float(wd_s[s]) * a + float(F32(eps)))
                if clip:
                    r = min(r / float(lr_s[s]), 1.0) if float(lr_s[s]) > 0 else 1.0
            rs[s] = r
            p.grad = r * (gt + float(wd_s[s]) * p.detach())
        opt.step()
        w = np.concatenate([p.detach().numpy() for p in ps])
        m = np.concatenate([opt.state[p]["momentum_buffer"].numpy() for p in ps])
        out.append((w.copy(), m.copy(), group_ref.per_element(rs, off)))
    return out


@pytest.mark.parametrize("clip", [0, 1])
@pytest.mark.parametrize("nesterov", [0, 1])
def test_the_restatement_follows_a_torch_lars_in_fp64_within_the_counted_roundings(nesterov, clip):
    """Three steps (the first with first = 1) of the restatement (sums of squares by math.fsum, the trust rule in fp64, the
    element rule in fp32) and of the torch LARS in fp64, from the same fp32 start, on the synthetic table with every tensor
    at its own eta and scales.  The bound is lars_ref.TorchBound: group_ref.TorchBound with two more roundings of 2^-24 on
    the trust-scaled term, and the ratio's own distance from n 2^-53 per norm and the carried error of w.  Nothing in it is
    fitted."""
    off = gc.synthetic()
    S = len(off) - 1
    hy, eta = grc.scales(S), lc.etas(S)
    lr, wd, mu, coef, gs, eps = 0.05, 5e-5, 0.9, 0.5, 0.5, lc.EPS
    lr_e, wd_e = _per_element(hy, off, lr, wd)
    w0, grads = gc.normals(N, 501), [gc.normals(N, 502 + k) for k in range(3)]
    ref = _torch_lars_three_steps(w0, grads, off, hy, eta, lr, wd, mu, coef, gs, eps, clip, nesterov)
    w, m = w0.copy(), np.zeros(N, F32)
    w64, m64 = w0.astype(np.float64), np.zeros(N)
    bound = lars_ref.TorchBound(N)
    seen = set()
    for k, g in enumerate(grads):
        trust = lars_ref.trust_rule(step_ref.stats(w, off)[0], step_ref.stats(g, off)[0], np.zeros(S, np.int32), eta,
                                    hy["lr_scale"], hy["wd_scale"], lr, wd, gs, coef, eps, clip)
        seen.update(np.flatnonzero(trust != 1.0).tolist())
        r = ref[k][2]
        bw, bm = bound.step(w64, g, m64, coef, lr_e, wd_e, r, bound.ratio_slack(w64, off), mu, gs, k == 0, nesterov)
        w, m = lars_ref.lars_rule(w, g, m, coef, lr_e, wd_e, group_ref.per_element(trust, off), mu, gs, k == 0, nesterov)
        w64, m64 = ref[k][0], ref[k][1]
        ew, em = np.abs(w.astype(np.float64) - w64), np.abs(m.astype(np.float64) - m64)
        print("step %d nesterov %d clip %d: max err w %.3g (bound %.3g at it), m %.3g (bound %.3g)"
              % (k, nesterov, clip, ew.max(), bw[ew.argmax()], em.max(), bm[em.argmax()]))
        assert np.all(ew <= bw) and np.all(em <= bm)
        assert np.all(trust[eta == 0] == 1.0)
    # with the clip most ratios of this table saturate at 1 (eta / lr_s is large); without it every eta > 0 shows
    assert len(seen) >= (1 if clip else int(np.count_nonzero(eta > 0)))


# -- the twins against the restatement ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("shifts", grc.SHIFTS, ids=lambda s: "shift%d%d%d" % s)
def test_lars_twins_equal_the_restatement(shifts):
    _lib()
    off = gc.synthetic()
    w0, m0 = gc.normals(N, 6), gc.normals(N, 7, 0.1)
    differ = 0
    for a in lc.GRID:
        h = lc.HostLars(off, shifts=shifts)
        g, max_norm = grc.gradient_for(a, N, 5)
        h.load(w0, g, m0)
        h.run(a, g, max_norm)
        cid = lc.case_id(a)
        assert h.coef() == (F32(0.5) if a["clipped"] else F32(1.0)), cid
        trust = _expected_trust(h, a)
        assert _bytes_equal(h.trust, trust), cid
        assert np.all(h.trust[h.eta == 0] == 1.0) and (a["clip"] or np.all(h.trust[h.eta > 0] != 1.0)), cid
        # the update's coefficient is 1 without a state (the gradient is then taken as it is)
        coef = h.coef() if a["state"] else F32(1.0)
        lr_e, wd_e = _per_element(h.hyper, off, gc.LR, a["wd"])
        w1, m1 = lars_ref.lars_rule(w0, g, m0, coef, lr_e, wd_e, group_ref.per_element(trust, off), a["mu"], a["gs"],
                                    a["first"], a["nesterov"])
        assert _bytes_equal(h.w, w1) and _bytes_equal(h.m, m1), cid
        assert _bytes_equal(h.g, g) and h.guards_intact(), cid
        assert int(h.state[_steplib.S_STEP]) == 1 and h.words() == (0, 0, 0)
        w2, _ = group_ref.group_rule(w0, g, m0, coef, lr_e, wd_e, a["mu"], a["gs"], a["first"], a["nesterov"])
        differ += not _bytes_equal(w1, w2)
    assert differ == len(lc.GRID), "the trust ratios show in every case"


def _one_step(off, shifts, seed, a):
    h = lc.HostLars(off, shifts=shifts)
    k = h.t.n
    g, w0, m0 = gc.normals(k, seed), gc.normals(k, seed + 1), gc.normals(k, seed + 2, 0.1)
    h.load(w0, g, m0)
    h.run(a, g)
    # wsumsq is what measure records on w at the same alignment, bytes equal
    ref = gc.HostGuard(off, shifts=(0, shifts[0], 0))
    ref.load(g=w0)
    ref.measure()
    rb = ref.t.record_bytes
    assert _bytes_equal(h.wsumsq, stepops.parse_record(ref.ring[:rb], ref.t.S)[1])
    trust = _expected_trust(h, a)
    assert _bytes_equal(h.trust, trust)
    lr_e, wd_e = _per_element(h.hyper, off, gc.LR, a["wd"])
    w1, m1 = lars_ref.lars_rule(w0, g, m0, h.coef(), lr_e, wd_e, group_ref.per_element(trust, off), a["mu"], a["gs"],
                                a["first"], a["nesterov"])
    assert _bytes_equal(h.w, w1) and _bytes_equal(h.m, m1) and _bytes_equal(h.g, g) and h.guards_intact()
    return h


@pytest.mark.parametrize("n", step_ref.EDGE_LENGTHS)
def test_lars_twins_on_every_edge_length(n):
    _lib()
    a = dict(first=0, gs=1.0, wd=5e-5, mu=0.9, nesterov=1, clip=0, state=True)
    for shifts in grc.SHIFTS:
        _one_step(step_ref.seg_off_of([n, 5, n]), shifts, 25, a)


@pytest.mark.parametrize("shifts", grc.SHIFTS, ids=lambda s: "shift%d%d%d" % s)
def test_lars_twins_on_tensors_around_a_group_an_item_and_many_items(shifts):
    _lib()
    a = dict(first=0, gs=0.5, wd=5e-5, mu=0.9, nesterov=0, clip=1, state=True)
    h = _one_step(lc.lengths_seg_off(), shifts, 45, a)
    assert int(h.t.seg_item[-1] - h.t.seg_item[-2]) == 71
    # the compensated item-order sum is within an ulp of the correctly rounded sum of the exact squares
    exact = step_ref.stats(gc.normals(h.t.n, 46), h.t.seg_off)[0]       # the weights before the step
    assert np.all(np.abs(h.wsumsq - exact) <= np.spacing(exact))


# -- identities ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shifts", [(0, 0, 0), (3, 3, 3), (0, 1, 2)], ids=lambda s: "shift%d%d%d" % s)
def test_wsumsq_is_the_sumsq_measure_host_records_on_w(shifts):
    _lib()
    off = gc.synthetic()
    h = lc.HostLars(off, shifts=shifts)
    w0 = gc.normals(N, 61)
    h.load(w0, gc.normals(N, 62), gc.normals(N, 63))
    h.measure()
    h.trust_host(dict(wd=5e-5, gs=1.0))
    ref = gc.HostGuard(off, shifts=(0, shifts[0], 0))
    ref.load(g=w0)
    ref.measure()
    assert _bytes_equal(h.wsumsq, stepops.parse_record(ref.ring[:ref.t.record_bytes], ref.t.S)[1])
    assert _bytes_equal(h.w, w0) and h.guards_intact()


@pytest.mark.parametrize("a", grc.GRID[::3], ids=grc.case_id)
def test_all_trust_one_is_apply_groups_host(a):
    _lib()
    off = gc.synthetic()
    g, max_norm = grc.gradient_for(a, N, 5)
    w0, m0 = gc.normals(N, 6), gc.normals(N, 7, 0.1)
    old, new = grc.HostGroup(off), lc.HostLars(off)
    for h in (old, new):
        h.load(w0, g, m0)
        if a["state"]:
            h.measure(max_norm)
    old.apply_groups(a, state=a["state"])
    new.apply_lars(a, state=a["state"], trust=np.ones(new.t.S, F32))
    assert _bytes_equal(new.w, old.w) and _bytes_equal(new.m, old.m) and _bytes_equal(new.state, old.state)
    assert not _bytes_equal(new.w, w0)


def test_eta_zero_zero_weights_and_zero_gradient_give_exactly_one():
    _lib()
    off = gc.synthetic()
    S = len(off) - 1
    eta = np.full(S, 0.01, F32)
    eta[3] = 0.0
    w0, g = gc.normals(N, 71), gc.normals(N, 72)
    w0[int(off[5]):int(off[6])] = 0.0
    g[int(off[7]):int(off[8])] = 0.0
    h = lc.HostLars(off, eta=eta)
    h.load(w0, g, gc.normals(N, 73))
    h.measure()
    h.trust_host(dict(wd=5e-5, gs=1.0))
    ones = [3, 5, 7]
    assert np.all(h.trust[ones].view(np.uint32) == 0x3f800000)
    assert np.all(np.delete(h.trust, ones) != 1.0) and h.wsumsq[5] == 0.0
    assert _bytes_equal(h.trust, _expected_trust(h, dict(wd=5e-5, gs=1.0)))


def test_with_a_clipping_coefficient_the_trust_uses_the_clipped_norm():
    _lib()
    off = gc.synthetic()
    a = dict(wd=0.0, gs=1.0, eps=0.0)
    w0, g = gc.normals(N, 81), gc.eights(N, 82)
    clipped, plain = lc.HostLars(off), lc.HostLars(off)
    for h, max_norm in ((clipped, 512.0), (plain, 0.0)):
        h.load(w0, g, gc.normals(N, 83))
        h.measure(max_norm)
        h.trust_host(a)
    assert clipped.coef() == F32(0.5) and plain.coef() == F32(1.0)
    assert _bytes_equal(clipped.trust, _expected_trust(clipped, a))
    on = clipped.eta > 0
    # half the gradient norm, no decay, no eps: twice the ratio, exactly (a power of two)
    assert np.array_equal(clipped.trust[on], plain.trust[on] * F32(2.0)) and np.all(clipped.trust[~on] == 1.0)


# -- non-finite values --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("value", [np.nan, np.inf, -np.inf], ids=["nan", "+inf", "-inf"])
def test_a_planted_nonfinite_gradient_gives_trust_one_and_the_guarded_update_is_skipped(value):
    _lib()
    off = gc.synthetic()
    a = dict(first=0, gs=1.0, wd=5e-5, mu=0.9, nesterov=1, clip=0, state=True)
    s = 9
    for shifts, at in (((0, 0, 0), int(off[s])), ((1, 1, 1), int(off[s + 1]) - 1), ((0, 1, 2), int(off[s]) + 7)):
        g, w0, m0 = gc.normals(N, 35), gc.normals(N, 36), gc.normals(N, 37, 0.1)
        g[at] = value
        h, old = lc.HostLars(off, shifts=shifts), gc.HostGuard(off, shifts=shifts)
        h.load(w0, g, m0)
        h.run(a, g, 1.0)
        assert h.trust[s] == 1.0 and _bytes_equal(h.trust, _expected_trust(h, a))
        assert _bytes_equal(h.w, w0) and _bytes_equal(h.m, m0) and _bytes_equal(h.g, g) and h.guards_intact()
        old.load(w0, g, m0)
        old.step(g, a, max_norm=1.0)
        assert h.words() == old.words() == (1, 1, 1) and _bytes_equal(h.state, old.state)


def test_a_planted_nan_in_w_gives_trust_one():
    _lib()
    off = gc.synthetic()
    w0 = gc.normals(N, 91)
    w0[int(off[10]) + 3] = np.nan
    w0[int(off[11]) + 5] = np.inf
    h = lc.HostLars(off)
    h.load(w0, gc.normals(N, 92), gc.normals(N, 93))
    h.measure()
    h.trust_host(dict(wd=5e-5, gs=1.0))
    assert np.isnan(h.wsumsq[10]) and np.isinf(h.wsumsq[11])
    assert h.trust[10] == 1.0 and h.trust[11] == 1.0 and h.eta[10] > 0 and h.eta[11] > 0
    assert np.all(np.isfinite(h.trust)) and _bytes_equal(h.trust, _expected_trust(h, dict(wd=5e-5, gs=1.0)))


# -- refusals -----------------------------------------------------------------------------------------------------------------
def _P(x):
    return x.ctypes.data


def _trust_args(h, **kw):
    return [kw.get("w", _P(h.w)), kw.get("n", h.t.n), kw.get("items", _P(h.t.items)), kw.get("seg_item", _P(h.t.seg_item)),
            kw.get("nitems", h.t.nitems), kw.get("hyper", _P(h.hyper)), kw.get("eta", _P(h.eta)), kw.get("S", h.t.S),
            kw.get("state", _P(h.state)), kw.get("ring", _P(h.ring)), kw.get("R", h.R), kw.get("ws", _P(h.tws)),
            kw.get("wsumsq", _P(h.wsumsq)), kw.get("trust", _P(h.trust)), 0.05, 5e-5, 1.0, kw.get("eps", 1e-8),
            kw.get("clip", 0)]


def _lars_args(h, **kw):
    return [kw.get("w", _P(h.w)), kw.get("g", _P(h.g)), kw.get("m", _P(h.m)), kw.get("n", h.t.n),
            kw.get("items", _P(h.t.items)), kw.get("nitems", h.t.nitems), kw.get("hyper", _P(h.hyper)),
            kw.get("trust", _P(h.trust)), kw.get("S", h.t.S), kw.get("state", _P(h.state)), kw.get("ring", _P(h.ring)),
            kw.get("R", h.R), 0.05, kw.get("mu", 0.9), 5e-5, 1.0, kw.get("first", 0), kw.get("nesterov", 0)]


def test_trust_refuses_what_it_cannot_run():
    L = _lib()
    h = lc.HostLars(step_ref.seg_off_of([5, 70, 2049]))
    n = h.t.n
    h.load(gc.normals(n, 1), gc.normals(n, 2), gc.normals(n, 3))
    out0 = (h.wsumsq.copy(), h.trust.copy(), h.tws.copy())
    assert L.x3dstep_trust_host(*_trust_args(h)) == -1                      # the step counter is 0
    assert b"nothing has been measured" in L.x3dstep_last_error()
    h.measure()
    state1, ring1 = h.state.copy(), h.ring.copy()
    gap = h.t.items.copy()
    gap["start"][1] += 1
    swapped = h.t.items.copy()
    swapped[[0, 1]] = swapped[[1, 0]]
    si = h.t.seg_item.copy()
    si[1] = 2
    bad = [dict(w=0), dict(items=0), dict(seg_item=0), dict(hyper=0), dict(eta=0), dict(state=0), dict(ring=0), dict(ws=0),
           dict(wsumsq=0), dict(trust=0), dict(n=0), dict(S=0), dict(R=0), dict(nitems=0), dict(w=_P(h.w) + 2),
           dict(eta=_P(h.eta) + 1), dict(trust=_P(h.trust) + 2), dict(wsumsq=_P(h.wsumsq) + 4), dict(ws=_P(h.tws) + 4),
           dict(state=_P(h.state) + 4), dict(items=_P(gap)), dict(items=_P(swapped)), dict(seg_item=_P(si)), dict(n=n + 1),
           dict(nitems=h.t.nitems - 1), dict(eps=-1e-8), dict(eps=np.nan), dict(eps=np.inf), dict(clip=2), dict(clip=-1)]
    for value in (-0.001, np.nan, np.inf, -np.inf):
        e = h.eta.copy()
        e[1] = value
        bad.append(dict(eta=_P(e), _keep=e))
    for field, value in (("lr_scale", -1.0), ("wd_scale", np.nan)):
        hy = h.hyper.copy()
        hy[field][2] = value
        bad.append(dict(hyper=_P(hy), _keep=hy))
    for kw in bad:
        assert L.x3dstep_trust_host(*_trust_args(h, **kw)) == -1, list(kw)
        assert b"x3dstep_trust_host" in L.x3dstep_last_error()
    assert _bytes_equal(h.wsumsq, out0[0]) and _bytes_equal(h.trust, out0[1]) and _bytes_equal(h.tws, out0[2])
    assert _bytes_equal(h.state, state1) and _bytes_equal(h.ring, ring1), "the state and the ring are only read"
    assert L.x3dstep_trust_host(*_trust_args(h)) == 0
    assert _bytes_equal(h.state, state1) and _bytes_equal(h.ring, ring1) and not _bytes_equal(h.trust, out0[1])
    with pytest.raises(ValueError):
        stepops.trust_host(h.w, h.t, h.hyper, h.eta[:-1], h.state, h.ring, h.R, h.tws, h.wsumsq, h.trust, 0.1)
    with pytest.raises(ValueError):
        stepops.trust_host(h.w, h.t, h.hyper, h.eta, h.state, h.ring, h.R, h.tws[:-1], h.wsumsq, h.trust, 0.1)
    with pytest.raises(ValueError):
        stepops.trust_host(h.w, h.t, h.hyper, h.eta, h.state, h.ring, h.R, h.tws, h.wsumsq.astype(F32), h.trust, 0.1)


def test_apply_lars_refuses_what_apply_groups_refuses_and_a_bad_trust():
    L = _lib()
    h = lc.HostLars(step_ref.seg_off_of([5, 70, 2049]))
    n = h.t.n
    h.load(gc.normals(n, 1), gc.normals(n, 2), gc.normals(n, 3))
    h.trust[:] = [0.5, 1.0, 2.0]
    before = (h.wbig.copy(), h.mbig.copy(), h.gbig.copy())
    assert L.x3dstep_apply_lars_host(*_lars_args(h)) == -1                  # the step counter is 0
    assert b"nothing has been measured" in L.x3dstep_last_error()
    h.measure()
    state1 = h.state.copy()
    short = h.t.items.copy()
    short["len"][-1] -= 1
    bad = [dict(w=0), dict(g=0), dict(m=0), dict(items=0), dict(hyper=0), dict(trust=0), dict(ring=0), dict(n=0), dict(R=0),
           dict(S=0), dict(nitems=0), dict(w=_P(h.w) + 2), dict(trust=_P(h.trust) + 2), dict(state=_P(h.state) + 4),
           dict(m=_P(h.w)), dict(g=_P(h.m) + 8), dict(items=_P(short)), dict(nitems=h.t.nitems - 1), dict(n=n + 1), dict(S=2),
           dict(first=2), dict(nesterov=-1), dict(nesterov=1, mu=0.0)]
    for value in (-0.5, np.nan, np.inf, -np.inf):
        t = h.trust.copy()
        t[1] = value
        bad.append(dict(trust=_P(t), _keep=t))
    hy = h.hyper.copy()
    hy["lr_scale"][1] = np.nan
    bad.append(dict(hyper=_P(hy), _keep=hy))
    for kw in bad:
        assert L.x3dstep_apply_lars_host(*_lars_args(h, **kw)) == -1, list(kw)
        assert b"x3dstep_apply_lars_host" in L.x3dstep_last_error()
    assert _bytes_equal(h.wbig, before[0]) and _bytes_equal(h.mbig, before[1]) and _bytes_equal(h.gbig, before[2])
    assert _bytes_equal(h.state, state1), "a refused call writes nothing"
    # the unguarded form needs neither state nor ring
    assert L.x3dstep_apply_lars_host(*_lars_args(h, state=0, ring=0, R=0)) == 0
    assert _bytes_equal(h.state, state1) and not _bytes_equal(h.wbig, before[0])
    assert L.x3dstep_apply_lars_host(*_lars_args(h)) == 0
    with pytest.raises(ValueError):
        stepops.apply_lars_host(h.w, h.g, h.m, h.t, h.hyper, h.trust[:-1], None, None, 0, 0.1)
    with pytest.raises(ValueError):
        stepops.apply_lars_host(h.w, h.g, h.m, h.t, h.hyper, h.trust, None, None, 0, 0.1, momentum=0.0, nesterov=True)


def test_the_twins_refuse_every_item_and_tensor_the_kernels_would_leave_out():
    """One bad item of each kind (tests/group_cases.py) and one bad tensor of each kind (tests/lars_cases.py): the twins,
    whose tables are host memory, refuse the call and write nothing.  That exactly that item or tensor is left untouched is
    shown on the per-item and per-tensor code itself by tests/lars_check.cpp and on the kernels by tests/test_lars_gpu.py."""
    L = _lib()
    h = lc.HostLars(gc.synthetic())
    h.load(gc.normals(N, 1), gc.normals(N, 2), gc.normals(N, 3))
    h.measure()
    h.trust[:] = 0.5
    before = (h.wbig.copy(), h.mbig.copy(), h.wsumsq.copy(), h.trust.copy())
    items = grc.bad_item_tables(h.t)
    assert len(items) == 10
    for name, it, hy, _ in items:
        assert L.x3dstep_apply_lars_host(*_lars_args(h, items=_P(it), hyper=_P(hy), state=0, ring=0, R=0)) == -1, name
        assert L.x3dstep_trust_host(*_trust_args(h, items=_P(it), hyper=_P(hy))) == -1, name
    tensors = lc.bad_tensor_tables(h.t)
    assert len(tensors) == 7
    for name, hy, eta, si, _ in tensors:
        assert L.x3dstep_trust_host(*_trust_args(h, hyper=_P(hy), eta=_P(eta), seg_item=_P(si))) == -1, name
    for value in (-1.0, np.nan, np.inf):
        t = h.trust.copy()
        t[9] = value
        assert L.x3dstep_apply_lars_host(*_lars_args(h, trust=_P(t), state=0, ring=0, R=0)) == -1
    assert all(_bytes_equal(x, y) for x, y in zip((h.wbig, h.mbig, h.wsumsq, h.trust), before))


# -- the same lists under the sanitisers --------------------------------------------------------------------------------------
def _write_case(f, off, R, shifts, hy, eta, steps, seed):
    """One case of tests/lars_check.cpp's file, with what the in-process twins gave as the expectation."""
    h = lc.HostLars(off, hyper=hy, eta=eta, R=R, shifts=shifts)
    n = h.t.n
    w0, m0 = gc.normals(n, seed), gc.normals(n, seed + 1, 0.1)
    h.load(w0, None, m0)
    f.write(struct.pack("<IIIIII", h.t.S, R, len(steps), *shifts))
    f.write(np.asarray(off, "<i8").tobytes())
    f.write(hy.tobytes() + eta.astype("<f4").tobytes())
    f.write(w0.astype("<f4").tobytes() + m0.astype("<f4").tobytes())
    for g, max_norm, a in steps:
        h.run(a, g, max_norm)
        f.write(struct.pack("<dfffffIIII", max_norm, gc.LR, a["mu"], a["wd"], a["gs"], a.get("eps", lc.EPS), a["first"],
                            a["nesterov"], 1 if a["state"] else 0, a["clip"]))
        f.write(g.astype("<f4").tobytes() + h.wsumsq.astype("<f8").tobytes() + h.trust.astype("<f4").tobytes())
        f.write(h.w.astype("<f4").tobytes() + h.m.astype("<f4").tobytes())
    f.write(h.state.astype("<i8").tobytes())


def test_the_same_lists_in_a_sanitised_stand_alone_program(tmp_path):
    """step_host.cpp and step_core.h compiled with -fsanitize=address,undefined into a program of their own
    (tests/lars_check.cpp), built and run as tests/group_check.cpp is: a child process, every buffer a heap block of
    exactly the size the library is told; nothing sanitised is loaded into this interpreter.  The program also runs the
    kernels' per-item and per-tensor code over the tables with one bad item or tensor each and checks that exactly that
    one is untouched."""
    step_program.compiler()
    _lib()
    syn = gc.synthetic()
    S = len(syn) - 1
    good, bad = gc.normals(N, 91), gc.normals(N, 92)
    bad[int(syn[9]) + 7] = np.nan
    base = dict(first=0, nesterov=1, mu=0.9, gs=0.5, wd=5e-5, clip=0, state=True, clipped=False)
    free = dict(base, state=False)
    cases = [(syn, 2, (0, 0, 0), grc.scales(S), lc.etas(S), [(good, 0.0, dict(base, first=1)), (bad, 1.0, base),
                                                             (good, 10.0, dict(base, clip=1)), (good, 0.0, free)], 400),
             (syn, 3, (1, 1, 1), grc.scales(S), lc.etas(S), [(gc.eights(N, 93), 512.0, dict(base, nesterov=0)),
                                                             (good, 0.0, dict(free, clip=1))], 410),
             (syn, 3, (3, 3, 3), grc.ones(S), np.zeros(S, F32), [(good, 10.0, dict(base, nesterov=0, mu=0.0))], 420),
             (syn, 3, (0, 1, 2), grc.scales(S), lc.etas(S), [(good, 10.0, base), (good, 0.0, free)], 430)]
    for n in step_ref.EDGE_LENGTHS:
        off = step_ref.seg_off_of([n, 5, n])
        cases.append((off, 1, (n % 4,) * 3, grc.scales(3), lc.etas(3) + F32(0.001), [(gc.normals(2 * n + 5, 94), 0.5, base)],
                      440 + n))
    off = lc.lengths_seg_off()
    k = int(off[-1])
    cases.append((off, 2, (2, 2, 2), grc.scales(len(off) - 1), lc.etas(len(off) - 1),
                  [(gc.normals(k, 95), 0.0, dict(base, clip=1)), (gc.normals(k, 96), 0.0, free)], 460))
    path = str(tmp_path / "lars_cases.bin")
    with open(path, "wb") as f:
        f.write(struct.pack("<I", len(cases)))
        for c in cases:
            _write_case(f, *c)
    last, out = step_program.run(tmp_path, "lars_check", path)
    assert last[:2] == ["lars", str(len(cases))] and last[2] == "items" and int(last[3]) == 13, out[-500:]
    assert last[4] == "tensors" and int(last[5]) == 7, out[-500:]
    assert int(last[-1]) == 0, out[-500:]
