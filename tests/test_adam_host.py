"""The second-moment updates of libx3dstep on the host: x3dstep_adam_host and the three x3dstep_lamb_*_host twins (the code
of the kernels through step_core.h) against the numpy restatement tests/adam_ref.py, byte for byte and inside guard bands,
with every tensor at its own scales; the restatement itself against torch.optim.AdamW / Adam and a LAMB in fp64; the powers
of the correction rule; the identities with x3dstep_measure_host; trusts of exactly 1; non-finite gradients under the guard;
the refusals; the ABI; the same lists in a sanitised stand-alone program.  No GPU."""
import math
import os
import re
import struct
import subprocess

import numpy as np
import pytest
import torch

from tests import adam_cases as ac
from tests import adam_ref, group_ref, step_ref
from tests import group_cases as grc
from tests import guard_cases as gc
from tests import lars_cases as lc
from tests import step_program
from x3dhip import _steplib, stepops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = ac.N
F32 = np.float32


def _lib():
    if not os.path.exists(_steplib.LIB_PATH):
        import __graft_entry__ as ge
        ge.build()
    return _steplib.lib()


def _bytes_equal(a, b):
    return np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


def _start(off, shifts, seed, hyper=None, adapt=None, R=4):
    """A HostAdam with w, m and v loaded, and copies of the three."""
    _lib()
    h = ac.HostAdam(off, hyper=hyper, adapt=adapt, R=R, shifts=shifts)
    n = h.t.n
    w0, m0, v0 = gc.normals(n, seed), gc.normals(n, seed + 1, 0.1), ac.second_moments(n, seed + 2)
    h.load(w0, None, m0, v0)
    return h, w0, m0, v0


def _measured_sumsq(x, off):
    """sumsq [S] as x3dstep_measure_host records it on x."""
    h = gc.HostGuard(off, R=1)
    h.load(g=x)
    h.measure()
    return stepops.parse_record(h.ring[:h.t.record_bytes], h.t.S)[1].copy()


def _check_case(h, a, off, w0, g, m0, v0, coef):
    """The twins' buffers after h.run(a, g) against the restatement."""
    e = ac.expected(a, off, h.hyper, h.adapt, w0, g, m0, v0, coef)
    assert _bytes_equal(h.m, e["m"]) and _bytes_equal(h.v, e["v"]), ac.case_id(a)
    if a["opt"] == "adam":
        assert _bytes_equal(h.w, e["w"]), ac.case_id(a)
    else:
        # the sums are what x3dstep_measure_host records on r and on w, bit for bit
        assert _bytes_equal(h.rsumsq, _measured_sumsq(e["r"], off)), ac.case_id(a)
        assert _bytes_equal(h.wsumsq, _measured_sumsq(w0, off)), ac.case_id(a)
        tr, w1 = e["finish"](h.wsumsq, h.rsumsq)
        assert _bytes_equal(h.trust, tr) and _bytes_equal(h.w, w1), ac.case_id(a)
    assert _bytes_equal(h.g, g) and h.guards_intact()


# -- ABI --------------------------------------------------------------------------------------------------------------------
def test_adam_header_ctypes_table_and_exports_agree():
    h = _lib()
    src = open(os.path.join(ROOT, "include", "x3dstep.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    nm = subprocess.run(["nm", "-D", "--defined-only", _steplib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exports = set(re.findall(r" T (x3dstep_[a-z0-9_]+)\n", nm))
    want = {"x3dstep_lamb_workspace_bytes": 1, "x3dstep_adam": 21, "x3dstep_adam_host": 20, "x3dstep_lamb_moments": 20,
            "x3dstep_lamb_moments_host": 19, "x3dstep_lamb_trust": 14, "x3dstep_lamb_trust_host": 13, "x3dstep_lamb_apply": 19,
            "x3dstep_lamb_apply_host": 18}
    for name, count in want.items():
        assert name in exports and name in _steplib.SIGNATURES
        decl = re.search(r"\b%s\s*\(([^)]*)\)" % name, code).group(1)
        assert len(decl.split(",")) == count == len(_steplib.SIGNATURES[name][1]), name
    # every declared symbol is exported and bound, and nothing else
    declared = set(re.findall(r"\b(x3dstep_[a-z0-9_]+)\s*\(", code))
    assert declared == exports == set(_steplib.SIGNATURES)
    assert h.x3dstep_abi_version() == 1 == _steplib.ABI_VERSION
    assert int(re.search(r"#define X3DSTEP_ABI_VERSION (\d+)", src).group(1)) == 1
    assert h.x3dstep_lamb_workspace_bytes(7) == 112 and h.x3dstep_lamb_workspace_bytes(0) == 0
    assert stepops.lamb_workspace_bytes(2092) == 16 * 2092
    with pytest.raises(ValueError):
        stepops.lamb_workspace_bytes(0)


# -- the correction rule ------------------------------------------------------------------------------------------------------
def test_the_powers_are_within_two_ulp_of_the_float_power():
    """pow_count of the restatement (the twins equal it through every grid case: bc1, bc2 feed every element) against
    Python's b ** k for k up to 10^6, underflow included.  Plain repeated squaring misses this by about k ulp."""
    rng = np.random.default_rng(5)
    ks = [0, 1, 2, 3, 7, 10, 100, 1000, 12345, 99999, 10 ** 5, 5 * 10 ** 5, 10 ** 6]
    ks += [int(k) for k in rng.integers(1, 10 ** 6, 600)] + list(range(700000, 750000, 997))
    worst = 0.0
    for b32 in (0.9, 0.99, 0.999, 0.9999, 0.99999, 0.95, 0.98, 0.8, 0.5, 1e-3, 0.0, float(np.nextafter(F32(1), F32(0)))):
        b = float(F32(b32))
        for k in ks:
            got, ref = adam_ref.pow_count(b, k), b ** k
            worst = max(worst, abs(got - ref) / math.ulp(ref))
    print("worst distance of the powers: %g ulp" % worst)
    assert worst <= 2.0


def test_the_twin_uses_the_restatements_powers_at_large_k():
    """One AdamW update as update k = 10^5 and 10^6: the correction terms come from the powers, so the bytes tell."""
    off = gc.synthetic()
    for k in (10 ** 5, 10 ** 6):
        a = dict(opt="adam", decoupled=1, gs=1.0, wd=0.01, state=False, clipped=False, k=k, betas=(0.99999, 0.9999))
        h, w0, m0, v0 = _start(off, (0, 0, 0, 0), 700)
        g = gc.normals(N, 703)
        h.run(a, g)
        _check_case(h, a, off, w0, g, m0, v0, 1.0)


# -- the twins against the restatement ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shifts", ac.SHIFTS, ids=ac.shift_id)
def test_adam_twins_equal_the_restatement(shifts):
    off = gc.synthetic()
    for i, a in enumerate(ac.GRID):
        h, w0, m0, v0 = _start(off, shifts, 100 + 3 * (i % 7))
        g, max_norm = ac.gradient_for(a, N, 200 + i)
        h.run(a, g, max_norm)
        coef = h.coef() if a["state"] else F32(1.0)
        assert (coef == F32(0.5)) == a["clipped"]
        _check_case(h, a, off, w0, g, m0, v0, coef)
        if a["state"]:
            assert h.words() == (0, 0, 0) and h.applied() == 1


def _one_step(off, shifts, seed, a):
    h, w0, m0, v0 = _start(off, shifts, seed, hyper=grc.scales(len(off) - 1))
    g = gc.normals(h.t.n, seed + 5)
    h.run(a, g, 0.5 if a["state"] else 0.0)
    _check_case(h, a, off, w0, g, m0, v0, h.coef() if a["state"] else F32(1.0))


EDGE_CASES = [dict(opt="adam", decoupled=1, gs=0.5, wd=0.01, state=True, clipped=False, k=3),
              dict(opt="adam", decoupled=0, gs=1.0, wd=0.01, state=False, clipped=False, k=1),
              dict(opt="lamb", decoupled=1, gs=0.5, wd=0.01, state=True, clipped=False, k=2)]


@pytest.mark.parametrize("n", step_ref.EDGE_LENGTHS)
def test_adam_twins_on_every_edge_length(n):
    off = step_ref.seg_off_of([n, 5, n])
    for a in EDGE_CASES:
        for s in (0, n % 4):
            _one_step(off, (s,) * 4, 300 + n, a)
        _one_step(off, (0, 1, 2, 3), 310 + n, a)


@pytest.mark.parametrize("shifts", ac.SHIFTS, ids=ac.shift_id)
def test_adam_twins_on_tensors_around_a_group_an_item_and_many_items(shifts):
    for a in EDGE_CASES:
        _one_step(lc.lengths_seg_off(), shifts, 320, a)


def test_subnormal_second_moments_and_a_denominator_of_eps():
    """Gradients so small that v' is subnormal (or 0) and sqrtf(v') / rbc2 vanishes against eps: den == eps exactly."""
    off = gc.synthetic()
    for a in (dict(opt="adam", decoupled=1, gs=1.0, wd=0.0, state=False, clipped=False, k=1, eps=1e-3),
              dict(opt="lamb", decoupled=1, gs=1.0, wd=0.0, state=False, clipped=False, k=1, eps=1e-3)):
        h = ac.HostAdam(off)
        w0 = gc.normals(N, 330)
        g = (gc.normals(N, 331) * F32(1e-19)).astype(F32)
        m0, v0 = np.zeros(N, F32), np.zeros(N, F32)
        h.load(w0, None, m0, v0)
        h.run(a, g)
        tiny = float(np.finfo(F32).tiny)
        assert np.count_nonzero((h.v > 0) & (h.v < tiny)) > N // 2          # subnormal second moments
        c = adam_ref.Corr(1, *ac.BETAS)
        assert np.all(np.sqrt(h.v) / c.rbc2 + F32(1e-3) == F32(1e-3))
        _check_case(h, a, off, w0, g, m0, v0, 1.0)


# -- the restatement against torch and against a LAMB in fp64 -------------------------------------------------------------------
def _torch_adam(dtype, decoupled, w0, grads, off, lr_s, wd_s, gs, betas, eps):
    """torch.optim.AdamW / Adam (single-tensor path) over the tensors of the buffer, every tensor its own group.  Gives
    (w, m, v) after the updates as fp64 arrays."""
    S = len(off) - 1
    ps = [torch.tensor(w0[int(off[s]):int(off[s + 1])], dtype=dtype, requires_grad=True) for s in range(S)]
    groups = [dict(params=[p], lr=float(lr_s[s]), weight_decay=float(wd_s[s])) for s, p in enumerate(ps)]
    cls = torch.optim.AdamW if decoupled else torch.optim.Adam
    opt = cls(groups, lr=1.0, betas=tuple(float(F32(b)) for b in betas), eps=float(F32(eps)), foreach=False)
    for g in grads:
        for s, p in enumerate(ps):
            p.grad = torch.tensor(g[int(off[s]):int(off[s + 1])], dtype=dtype) * float(F32(gs))
        opt.step()
    cat = lambda key: np.concatenate([opt.state[p][key].double().numpy() for p in ps])          # noqa: E731
    return np.concatenate([p.detach().double().numpy() for p in ps]), cat("exp_avg"), cat("exp_avg_sq")


@pytest.mark.parametrize("decoupled", [1, 0], ids=["adamw", "adam"])
def test_the_restatement_follows_torch_adam_in_fp64(decoupled):
    """Five updates from zero moments.  The quotient m' / den cannot be bounded by counted roundings in closed form (the
    denominator's relative error depends on sqrt(v') against eps), so the yardstick is torch's own fp32 single-tensor run:
    its distance from the fp64 run on the same inputs, and four times that allowed for the restatement, whose order of
    operations differs from torch's by a few roundings per update (the folded step size, w * (1 - lr wd) as one fma), not
    by a term that grows.  With AdamW the moments do not depend on w and their roundings are counted as test_lars_host
    counts: m' has four (t, 1 - b1, the product, the fma) relative to M = b1 |m| + (1 - b1) |t|, v' six (t twice, t * t,
    1 - b2, the product, the fma) relative to V, carried by b1 and b2."""
    off = gc.synthetic()
    hy = grc.scales(len(off) - 1)
    lr, wd, gs, eps = 0.01, 0.01, 0.5, 1e-8
    lr_t, wd_t = group_ref.tensor_rule(lr, wd, hy["lr_scale"], hy["wd_scale"])
    lr_s, wd_s = ac.per_element(hy, off, lr, wd)
    w0 = gc.normals(N, 400)
    grads = [gc.normals(N, 401 + i) for i in range(5)]
    w64, m64, v64 = _torch_adam(torch.float64, decoupled, w0, grads, off, lr_t, wd_t, gs, ac.BETAS, eps)
    w32, m32, v32 = _torch_adam(torch.float32, decoupled, w0, grads, off, lr_t, wd_t, gs, ac.BETAS, eps)
    w, m, v = w0.copy(), np.zeros(N, F32), np.zeros(N, F32)
    b1, b2 = float(F32(ac.BETAS[0])), float(F32(ac.BETAS[1]))
    em, ev = np.zeros(N), np.zeros(N)
    md, vd = np.zeros(N), np.zeros(N)
    slack = 1.0 + 2.0 ** -20
    for k, g in enumerate(grads, 1):
        w, m, v = adam_ref.adam_rule(w, g, m, v, 1.0, lr_s, wd_s, k, ac.BETAS[0], ac.BETAS[1], eps, gs, decoupled)
        if decoupled:
            t = g.astype(np.float64) * gs
            em = b1 * em + 4 * group_ref.EPS * (b1 * np.abs(md) + (1 - b1) * np.abs(t)) * slack
            ev = b2 * ev + 6 * group_ref.EPS * (b2 * vd + (1 - b2) * t * t) * slack
            md, vd = b1 * md + (1 - b1) * t, b2 * vd + (1 - b2) * t * t
    if decoupled:
        assert np.all(np.abs(m.astype(np.float64) - m64) <= em + 1e-300)
        assert np.all(np.abs(v.astype(np.float64) - v64) <= ev + 1e-300)
    for name, ours, t32, t64 in (("w", w, w32, w64), ("m", m, m32, m64), ("v", v, v32, v64)):
        d_ours = float(np.max(np.abs(ours.astype(np.float64) - t64)))
        d_torch = float(np.max(np.abs(t32 - t64)))
        print("%s %s: restatement %.3e, torch fp32 %.3e from torch fp64: ratio %.3f"
              % ("adamw" if decoupled else "adam", name, d_ours, d_torch, d_ours / d_torch))
        assert d_ours <= 4.0 * d_torch


def _plain_lamb(dtype, w0, grads, off, lr_s, wd_s, adapt, gs, betas, eps):
    """LAMB (You et al. 2020) in plain numpy at one precision: (w, m, v) as fp64 arrays."""
    cast = lambda x: np.asarray(x).astype(dtype)                                                  # noqa: E731
    b1, b2, eps, gs = (dtype(float(F32(x))) for x in (betas[0], betas[1], eps, gs))
    lr_s, wd_s = cast(lr_s), cast(wd_s)
    w, m, v = cast(w0), np.zeros(len(w0), dtype), np.zeros(len(w0), dtype)
    for k, g in enumerate(grads, 1):
        t = cast(g) * gs
        m, v = b1 * m + (1 - b1) * t, b2 * v + (1 - b2) * t * t
        r = (m / (1 - b1 ** k)) / (np.sqrt(v / (1 - b2 ** k)) + eps) + wd_s * w
        tr = np.ones(len(off) - 1, dtype)
        for s in range(len(off) - 1):
            sl = slice(int(off[s]), int(off[s + 1]))
            a, b = np.sqrt(np.sum(w[sl] * w[sl])), np.sqrt(np.sum(r[sl] * r[sl]))
            if adapt[s] and a > 0 and b > 0:
                tr[s] = a / b
        w = w - lr_s * group_ref.per_element(tr, off) * r
    return w.astype(np.float64), m.astype(np.float64), v.astype(np.float64)


def test_the_restatement_follows_a_lamb_in_fp64():
    """The same way as for Adam: five updates of the 20-line LAMB above in fp64 and in fp32, and the restatement (with the
    correctly rounded sums of squares in the place of the library's ordered ones: the order costs 2^-53 per term) within
    four times the fp32 run's distance from the fp64 run."""
    off = gc.synthetic()
    S = len(off) - 1
    hy, adapt = grc.scales(S), ac.adapts(S)
    lr, wd, gs, eps = 0.01, 0.01, 0.5, 1e-6
    lr_s, wd_s = ac.per_element(hy, off, lr, wd)
    w0 = gc.normals(N, 420)
    grads = [gc.normals(N, 421 + i) for i in range(5)]
    w64, m64, v64 = _plain_lamb(np.float64, w0, grads, off, lr_s, wd_s, adapt, gs, ac.BETAS, eps)
    w32, m32, v32 = _plain_lamb(np.float32, w0, grads, off, lr_s, wd_s, adapt, gs, ac.BETAS, eps)
    w, m, v = w0.copy(), np.zeros(N, F32), np.zeros(N, F32)
    for k, g in enumerate(grads, 1):
        m, v, r = adam_ref.lamb_moments(w, g, m, v, 1.0, wd_s, k, ac.BETAS[0], ac.BETAS[1], eps, gs)
        tr = adam_ref.lamb_trust(step_ref.stats(w, off)[0], step_ref.stats(r, off)[0], adapt, np.zeros(S, np.int32))
        w = adam_ref.lamb_apply(w, r, lr_s, group_ref.per_element(tr, off))
    for name, ours, t32, t64 in (("w", w, w32, w64), ("m", m, m32, m64), ("v", v, v32, v64)):
        d_ours = float(np.max(np.abs(ours.astype(np.float64) - t64)))
        d_plain = float(np.max(np.abs(t32 - t64)))
        print("lamb %s: restatement %.3e, plain fp32 %.3e from plain fp64: ratio %.3f" % (name, d_ours, d_plain, d_ours / d_plain))
        assert d_ours <= 4.0 * d_plain


# -- trusts of exactly one ------------------------------------------------------------------------------------------------------
def test_adapt_zero_zero_weights_and_a_zero_direction_give_exactly_one():
    off = gc.synthetic()
    S = len(off) - 1
    a = dict(opt="lamb", decoupled=1, gs=1.0, wd=0.0, state=False, clipped=False, k=1)
    h, w0, m0, v0 = _start(off, (0, 0, 0, 0), 500, hyper=grc.ones(S))
    adapt = np.ones(S, np.uint8)
    adapt[3] = 0                                           # exempt
    h.adapt = adapt
    g = gc.normals(N, 503)
    w0[int(off[5]):int(off[6])] = 0.0                      # zero weights
    sl = slice(int(off[7]), int(off[8]))                   # a zero direction: no gradient, no momentum, no decay
    g[sl] = 0.0
    m0[sl] = 0.0
    h.load(w0, None, m0, v0)
    h.run(a, g)
    assert h.rsumsq[7] == 0.0 and h.wsumsq[5] == 0.0
    for s in (3, 5, 7):
        assert h.trust[s].tobytes() == F32(1.0).tobytes()
    assert np.all(h.trust[[s for s in range(S) if s not in (3, 5, 7)]] != F32(1.0))
    assert _bytes_equal(h.w[sl], w0[sl])
    _check_case(h, a, off, w0, g, m0, v0, 1.0)


# -- non-finite gradients under the guard -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("opt", ["adam", "lamb"])
@pytest.mark.parametrize("value", [np.nan, np.inf, -np.inf], ids=["nan", "+inf", "-inf"])
def test_a_planted_nonfinite_gradient_is_skipped_and_does_not_advance_the_correction(opt, value):
    off = gc.synthetic()
    a = dict(opt=opt, decoupled=1, gs=1.0, wd=0.01, state=True, clipped=False, k=1)
    h, w0, m0, v0 = _start(off, (0, 0, 0, 0), 520)
    run = h.lamb if opt == "lamb" else h.adam
    bad, good = gc.normals(N, 523), gc.normals(N, 524)
    bad[int(off[9]) + 7] = value
    h.trust[:] = 1.0                                       # as the trainer starts it: the twin refuses a trust that is not one
    outs = (h.wsumsq.copy(), h.rsumsq.copy(), h.trust.copy(), h.lws.copy())
    h.load(g=bad)
    h.measure()
    run(a, 0)
    assert _bytes_equal(h.w, w0) and _bytes_equal(h.m, m0) and _bytes_equal(h.v, v0) and h.words() == (1, 1, 1)
    assert all(_bytes_equal(x, y) for x, y in zip((h.wsumsq, h.rsumsq, h.trust, h.lws), outs))
    # the next applied update is update 1, as if the skipped one had never happened
    h.load(g=good)
    h.measure()
    run(a, 0)
    assert h.words() == (0, 1, 0) and h.applied() == 1
    fresh, _, _, _ = _start(off, (0, 0, 0, 0), 520)
    fresh.trust[:] = 1.0
    fresh.run(a, good)
    assert fresh.count_for(a) == 0
    for x, y in ((h.w, fresh.w), (h.m, fresh.m), (h.v, fresh.v), (h.trust, fresh.trust)):
        assert _bytes_equal(x, y)
    _check_case(h, a, off, w0, good, m0, v0, 1.0)


# -- refusals -------------------------------------------------------------------------------------------------------------------
def _P(x):
    return x.ctypes.data


def _adam_args(h, **kw):
    d = dict(w=_P(h.w), g=_P(h.g), m=_P(h.m), v=_P(h.v), n=h.t.n, items=_P(h.t.items), nitems=h.t.nitems, hyper=_P(h.hyper),
             S=h.t.S, state=_P(h.state), ring=_P(h.ring), R=h.R, count=0, lr=0.01, b1=0.9, b2=0.999, eps=1e-8, wd=0.01, gs=1.0,
             decoupled=1)
    d.update(kw)
    return [d[k] for k in ("w", "g", "m", "v", "n", "items", "nitems", "hyper", "S", "state", "ring", "R", "count", "lr", "b1",
                           "b2", "eps", "wd", "gs", "decoupled")]


def _moments_args(h, **kw):
    d = dict(w=_P(h.w), g=_P(h.g), m=_P(h.m), v=_P(h.v), n=h.t.n, items=_P(h.t.items), nitems=h.t.nitems, hyper=_P(h.hyper),
             S=h.t.S, state=_P(h.state), ring=_P(h.ring), R=h.R, count=0, b1=0.9, b2=0.999, eps=1e-6, wd=0.01, gs=1.0,
             ws=_P(h.lws))
    d.update(kw)
    return [d[k] for k in ("w", "g", "m", "v", "n", "items", "nitems", "hyper", "S", "state", "ring", "R", "count", "b1", "b2",
                           "eps", "wd", "gs", "ws")]


def _trust_args(h, **kw):
    d = dict(seg_item=_P(h.t.seg_item), nitems=h.t.nitems, hyper=_P(h.hyper), adapt=_P(h.adapt), S=h.t.S, state=_P(h.state),
             ring=_P(h.ring), R=h.R, count=0, ws=_P(h.lws), wsumsq=_P(h.wsumsq), rsumsq=_P(h.rsumsq), trust=_P(h.trust))
    d.update(kw)
    return [d[k] for k in ("seg_item", "nitems", "hyper", "adapt", "S", "state", "ring", "R", "count", "ws", "wsumsq", "rsumsq",
                           "trust")]


def _apply_args(h, **kw):
    d = dict(w=_P(h.w), m=_P(h.m), v=_P(h.v), n=h.t.n, items=_P(h.t.items), nitems=h.t.nitems, hyper=_P(h.hyper),
             trust=_P(h.trust), S=h.t.S, state=_P(h.state), ring=_P(h.ring), R=h.R, count=0, lr=0.01, b1=0.9, b2=0.999, eps=1e-6,
             wd=0.01)
    d.update(kw)
    return [d[k] for k in ("w", "m", "v", "n", "items", "nitems", "hyper", "trust", "S", "state", "ring", "R", "count", "lr", "b1",
                           "b2", "eps", "wd")]


def _measured(seed=600):
    h, _, _, _ = _start(gc.synthetic(), (0, 0, 0, 0), seed)
    h.load(g=gc.normals(N, seed + 3))
    h.measure()
    h.trust[:] = 1.0
    return h


def _everything(h):
    return [x.copy() for x in (h.wbig, h.gbig, h.mbig, h.vbig, h.state, h.lws, h.wsumsq, h.rsumsq, h.trust)]


def _untouched(h, before):
    return all(_bytes_equal(x, y) for x, y in zip((h.wbig, h.gbig, h.mbig, h.vbig, h.state, h.lws, h.wsumsq, h.rsumsq, h.trust),
                                                  before))


def test_every_refusal_writes_nothing():
    L = _lib()
    h = _measured()
    before = _everything(h)
    nan = float("nan")
    common = [dict(v=0), dict(v=_P(h.v) + 2), dict(v=_P(h.w)), dict(v=_P(h.m) + 64), dict(w=0), dict(m=0), dict(n=0),
              dict(items=0), dict(items=_P(h.t.items) + 4), dict(nitems=0), dict(hyper=0), dict(S=0), dict(ring=0), dict(R=0),
              dict(state=_P(h.state) + 4), dict(b1=1.0), dict(b1=-0.1), dict(b1=nan), dict(b2=1.0), dict(b2=-0.1), dict(b2=nan),
              dict(eps=-1e-8), dict(eps=nan), dict(eps=float("inf")), dict(count=-1), dict(count=-5),
              dict(state=0, ring=0, R=0, count=0), dict(state=0, ring=0, R=0, count=-3)]
    for kw in common + [dict(g=0), dict(v=_P(h.g)), dict(decoupled=2), dict(decoupled=-1)]:
        assert L.x3dstep_adam_host(*_adam_args(h, **kw)) == -1, kw
        assert _untouched(h, before), kw
    for kw in common + [dict(g=0), dict(v=_P(h.g)), dict(ws=0), dict(ws=_P(h.lws) + 4)]:
        assert L.x3dstep_lamb_moments_host(*_moments_args(h, **kw)) == -1, kw
        assert _untouched(h, before), kw
    for kw in common + [dict(trust=0), dict(trust=_P(h.trust) + 2)]:
        assert L.x3dstep_lamb_apply_host(*_apply_args(h, **kw)) == -1, kw
        assert _untouched(h, before), kw
    for kw in (dict(seg_item=0), dict(hyper=0), dict(adapt=0), dict(ws=0), dict(wsumsq=0), dict(rsumsq=0), dict(trust=0),
               dict(rsumsq=_P(h.wsumsq)), dict(S=0), dict(nitems=h.t.S - 1), dict(ring=0), dict(R=0), dict(count=-1),
               dict(state=0, ring=0, R=0, count=0), dict(wsumsq=_P(h.wsumsq) + 4)):
        assert L.x3dstep_lamb_trust_host(*_trust_args(h, **kw)) == -1, kw
        assert _untouched(h, before), kw
    # a counter of 0: nothing has been measured
    fresh, _, _, _ = _start(gc.synthetic(), (0, 0, 0, 0), 610)
    fresh.trust[:] = 1.0
    before = _everything(fresh)
    for fn, args in ((L.x3dstep_adam_host, _adam_args(fresh, count=1)), (L.x3dstep_lamb_moments_host, _moments_args(fresh, count=1)),
                     (L.x3dstep_lamb_trust_host, _trust_args(fresh, count=1)), (L.x3dstep_lamb_apply_host, _apply_args(fresh, count=1))):
        assert fn(*args) == -1
        assert _untouched(fresh, before)
    # the python wrappers refuse before anything is called
    with pytest.raises(ValueError):
        stepops._adam_args("adam", (0.9, 1.0), 1e-8)
    with pytest.raises(ValueError):
        stepops._adam_args("adam", (0.9, 0.999), -1.0)


def test_the_twins_refuse_every_item_and_tensor_the_kernels_would_leave_out():
    L = _lib()
    h = _measured(620)
    before = _everything(h)
    for name, items, hy, _ in grc.bad_item_tables(h.t):
        for fn, args in ((L.x3dstep_adam_host, _adam_args), (L.x3dstep_lamb_moments_host, _moments_args),
                         (L.x3dstep_lamb_apply_host, _apply_args)):
            assert fn(*args(h, items=_P(items), hyper=_P(hy))) == -1, name
            assert _untouched(h, before), name
    for value in (-1.0, np.nan, np.inf):
        t = h.trust.copy()
        t[9] = value
        assert L.x3dstep_lamb_apply_host(*_apply_args(h, trust=_P(t))) == -1
    for name, hy, _, si, _ in lc.bad_tensor_tables(h.t):
        if name.startswith("eta"):
            continue
        assert L.x3dstep_lamb_trust_host(*_trust_args(h, hyper=_P(hy), seg_item=_P(si))) == -1, name
        assert _untouched(h, before), name


# -- the same lists under the sanitisers --------------------------------------------------------------------------------------
def _write_case(f, off, R, shifts, hy, adapt, steps, seed):
    """One case of tests/adam_check.cpp's file, with what the in-process twins gave as the expectation."""
    h, w0, m0, v0 = _start(off, shifts, seed, hyper=hy, adapt=adapt, R=R)
    f.write(struct.pack("<IIIIIII", h.t.S, R, len(steps), *shifts))
    f.write(np.asarray(off, "<i8").tobytes() + hy.tobytes() + adapt.astype(np.uint8).tobytes())
    f.write(w0.astype("<f4").tobytes() + m0.astype("<f4").tobytes() + v0.astype("<f4").tobytes())
    for g, max_norm, a in steps:
        h.load(g=g)
        if a["state"]:
            h.measure(max_norm)
        count = h.count_for(a)
        (h.lamb if a["opt"] == "lamb" else h.adam)(a, count, state=a["state"])
        f.write(struct.pack("<dqffffffIII", max_norm, count, ac.LR, ac.BETAS[0], ac.BETAS[1], ac.EPS[a["opt"]], a["wd"], a["gs"],
                            1 if a["opt"] == "lamb" else 0, a["decoupled"], 1 if a["state"] else 0))
        f.write(g.astype("<f4").tobytes() + h.w.astype("<f4").tobytes() + h.m.astype("<f4").tobytes() + h.v.astype("<f4").tobytes())
        f.write(h.wsumsq.astype("<f8").tobytes() + h.rsumsq.astype("<f8").tobytes() + h.trust.astype("<f4").tobytes())
    f.write(h.state.astype("<i8").tobytes())


def test_the_same_lists_in_a_sanitised_stand_alone_program(tmp_path):
    """step_host.cpp and step_core.h compiled with -fsanitize=address,undefined into a program of their own
    (tests/adam_check.cpp), built and run as tests/lars_check.cpp is: a child process, every buffer a heap block of exactly
    the size the library is told; nothing sanitised is loaded into this interpreter.  The program also runs the kernels'
    per-item code over the tables with one bad item each and checks that exactly that one is untouched."""
    step_program.compiler()
    _lib()
    syn = gc.synthetic()
    S = len(syn) - 1
    good, bad = gc.normals(N, 91), gc.normals(N, 92)
    bad[int(syn[9]) + 7] = np.nan
    aw = dict(opt="adam", decoupled=1, gs=0.5, wd=0.01, state=True, clipped=False, k=1)
    ad = dict(aw, decoupled=0)
    lb = dict(aw, opt="lamb")
    k2 = lambda a, k, **kw: dict(a, k=k, **kw)                                                     # noqa: E731
    cases = [(syn, 2, (0, 0, 0, 0), grc.scales(S), ac.adapts(S), [(good, 0.0, aw), (bad, 1.0, k2(aw, 2)), (good, 10.0, k2(aw, 2)),
                                                                (good, 0.0, k2(ad, 7, state=False))], 800),
             (syn, 3, (1, 1, 1, 1), grc.scales(S), ac.adapts(S), [(gc.eights(N, 93), 512.0, lb), (bad, 0.0, k2(lb, 2)),
                                                                (good, 0.0, k2(lb, 2)), (good, 0.0, k2(lb, 1000, state=False))], 810),
             (syn, 3, (3, 3, 3, 3), grc.ones(S), np.zeros(S, np.uint8), [(good, 10.0, lb), (good, 0.0, k2(ad, 2))], 820),
             (syn, 3, (0, 1, 2, 3), grc.scales(S), ac.adapts(S), [(good, 10.0, aw), (good, 0.0, k2(lb, 2))], 830),
             (syn, 3, (1, 0, 0, 0), grc.scales(S), ac.adapts(S), [(good, 10.0, lb)], 835)]
    for n in step_ref.EDGE_LENGTHS:
        off = step_ref.seg_off_of([n, 5, n])
        cases.append((off, 1, (n % 4,) * 4, grc.scales(3), np.ones(3, np.uint8),
                      [(gc.normals(2 * n + 5, 94), 0.5, aw), (gc.normals(2 * n + 5, 95), 0.5, k2(lb, 2))], 840 + n))
    off = lc.lengths_seg_off()
    k = int(off[-1])
    cases.append((off, 2, (2, 2, 2, 2), grc.scales(len(off) - 1), ac.adapts(len(off) - 1),
                  [(gc.normals(k, 95), 0.0, lb), (gc.normals(k, 96), 0.0, k2(aw, 2, state=False))], 860))
    path = str(tmp_path / "adam_cases.bin")
    with open(path, "wb") as f:
        f.write(struct.pack("<I", len(cases)))
        for c in cases:
            _write_case(f, *c)
    last, out = step_program.run(tmp_path, "adam_check", path)
    assert last[:2] == ["adam", str(len(cases))] and last[2] == "items" and int(last[3]) == 10, out[-500:]
    assert int(last[-1]) == 0, out[-500:]
