"""The guarded update of libx3dstep on the host: x3dstep_measure_host, x3dstep_apply_host and x3dstep_keep_host (the code of
the kernels through step_core.h) against the numpy restatement tests/guard_ref.py, byte for byte and inside guard bands;
the skip decision and its counters; the refusals; the ABI; the same lists in a sanitised stand-alone program.  No GPU."""
import ctypes
import os
import re
import struct
from fractions import Fraction

import numpy as np
import pytest

from tests import guard_cases as gc
from tests import guard_ref, step_ref
from tests import step_program
from x3dhip import _steplib, stepops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 16384


def _lib():
    if not os.path.exists(_steplib.LIB_PATH):
        import __graft_entry__ as ge
        ge.build()
    return _steplib.lib()


def _bytes_equal(a, b):
    return np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


# -- ABI --------------------------------------------------------------------------------------------------------------------
def test_guard_header_ctypes_table_and_constants_agree():
    h = _lib()
    src = open(os.path.join(ROOT, "include", "x3dstep.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    funcs = sorted(set(re.findall(r"\b(x3dstep_[a-z0-9_]+)\s*\(", code)))
    assert funcs == sorted(_steplib.SIGNATURES.keys())
    for name in ("x3dstep_measure", "x3dstep_measure_host", "x3dstep_apply", "x3dstep_apply_host", "x3dstep_keep",
                 "x3dstep_keep_host"):
        assert name in funcs
        # the argument count of the declaration is the ctypes table's
        decl = re.search(r"\b%s\s*\(([^)]*)\)" % name, code).group(1)
        assert len(decl.split(",")) == len(_steplib.SIGNATURES[name][1]), name
    for name, val in (("S_SKIP", _steplib.S_SKIP), ("S_SKIPPED", _steplib.S_SKIPPED), ("S_RUN", _steplib.S_RUN),
                      ("KEEP_SAVE", _steplib.KEEP_SAVE), ("KEEP_RESTORE", _steplib.KEEP_RESTORE),
                      ("STATE_WORDS", _steplib.STATE_WORDS), ("ABI_VERSION", _steplib.ABI_VERSION)):
        assert int(re.search(r"#define X3DSTEP_%s (\d+)" % name, src).group(1)) == val, name
    assert (_steplib.S_SKIP, _steplib.S_SKIPPED, _steplib.S_RUN) == (5, 6, 7) and _steplib.STATE_WORDS == 8
    assert h.x3dstep_abi_version() == 1 and h.x3dstep_header_bytes() == 40
    assert h.x3dstep_keep_bytes() == _steplib.KEEP_DT.itemsize == 24
    assert stepops.new_state()[5:].tolist() == [0, 0, 0]


# -- the restatement itself ---------------------------------------------------------------------------------------------------
def test_the_vectorised_fma_of_the_restatement_is_the_exact_one():
    rng = np.random.default_rng(3)
    a = rng.standard_normal(400).astype(np.float32)
    b = (rng.standard_normal(400) * 1e-3).astype(np.float32)
    c = rng.standard_normal(400).astype(np.float32)
    # ties of the fp32 grid that only the exact sum resolves: 1 + 2^-24 (+- a product far below fp64's last bit)
    a[:4] = np.float32(2.0 ** -24)
    b[:4] = [1.0, 1.0, 1.0, 1.0]
    c[:4] = [1.0, 1.0 + 2.0 ** -23, -1.0, 3.0]
    a[4:8] = np.float32(2.0 ** -60)
    b[4:8] = [1.0, -1.0, 1.0, -1.0]
    c[4:8] = np.float32(1.0) + np.float32(2.0 ** -23) * np.array([0, 0, 1, 1], np.float32)
    a[8:10], b[8:10], c[8:10] = [0.0, -0.0], [1.0, 1.0], [-0.0, -0.0]       # exact zeros: the sign rule
    got = guard_ref.fma_f32(a, b, c)
    want = np.array([guard_ref.fma_exact(x, y, z) for x, y, z in zip(a, b, c)], np.float32)
    assert _bytes_equal(got, want)
    assert got[0] == np.float32(1.0) and got[1] == np.float32(1.0 + 2.0 ** -22)          # ties to even
    assert guard_ref.round_f32(Fraction(1) + Fraction(1, 2 ** 24) + Fraction(1, 2 ** 80)) == np.float32(1.0 + 2.0 ** -23)
    assert np.signbit(got[9]) and not np.signbit(got[8])


# -- arithmetic: the twin against the restatement ---------------------------------------------------------------------------
@pytest.mark.parametrize("a", gc.ARITH, ids=gc.arith_id)
def test_apply_twin_equals_the_restatement(a):
    _lib()
    h = gc.HostGuard(gc.synthetic())
    g, max_norm = gc.gradient_for(a, N, 5)
    w0, m0 = gc.normals(N, 6), gc.normals(N, 7, 0.1)
    h.load(w0, g, m0)
    h.measure(max_norm)
    coef = h.coef()
    assert coef == (np.float32(0.5) if a["clipped"] else np.float32(1.0))
    h.apply(a)
    w1, m1 = guard_ref.apply_rule(w0, g, m0, coef, gc.LR, a["mu"], a["wd"], a["gs"], a["first"])
    assert _bytes_equal(h.w, w1) and _bytes_equal(h.m, m1)
    assert _bytes_equal(h.g, g), "g is not written: the scaled gradient exists in registers only"
    assert h.words() == (0, 0, 0) and h.guards_intact()
    assert not _bytes_equal(w1, w0)


@pytest.mark.parametrize("shifts", [(0, 0, 0), (1, 1, 1), (2, 2, 2), (3, 3, 3), (0, 1, 2)],
                         ids=lambda s: "shift%d%d%d" % s)
def test_apply_twin_at_every_alignment(shifts):
    _lib()
    a = dict(first=0, gs=0.5, wd=5e-5, mu=0.9)
    h = gc.HostGuard(gc.synthetic(), shifts=shifts)
    g, w0, m0 = gc.normals(N, 15), gc.normals(N, 16), gc.normals(N, 17, 0.1)
    h.load(w0, g, m0)
    h.measure(10.0)
    coef = h.coef()
    assert 0.0 < coef < 1.0                              # norm about 128
    h.apply(a)
    w1, m1 = guard_ref.apply_rule(w0, g, m0, coef, gc.LR, a["mu"], a["wd"], a["gs"], a["first"])
    assert _bytes_equal(h.w, w1) and _bytes_equal(h.m, m1) and _bytes_equal(h.g, g) and h.guards_intact()


@pytest.mark.parametrize("n", step_ref.EDGE_LENGTHS)
def test_apply_twin_on_every_edge_length(n):
    """One tensor of each length of the step tests' table as the whole buffer: heads, tails and groups of every size."""
    _lib()
    a = dict(first=0, gs=1.0, wd=5e-5, mu=0.9)
    for shifts in ((0, 0, 0), (1, 1, 1), (2, 2, 2), (3, 3, 3), (2, 0, 1)):
        h = gc.HostGuard(step_ref.seg_off_of([n]), shifts=shifts)
        g, w0, m0 = gc.normals(n, 25), gc.normals(n, 26), gc.normals(n, 27, 0.1)
        h.load(w0, g, m0)
        h.measure(0.5)
        h.apply(a)
        w1, m1 = guard_ref.apply_rule(w0, g, m0, h.coef(), gc.LR, a["mu"], a["wd"], a["gs"], a["first"])
        assert _bytes_equal(h.w, w1) and _bytes_equal(h.m, m1) and _bytes_equal(h.g, g) and h.guards_intact()


# -- the skip decision ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("value", [np.nan, np.inf, -np.inf], ids=["nan", "+inf", "-inf"])
def test_one_nonfinite_element_leaves_w_and_m_untouched(value):
    _lib()
    a = dict(first=0, gs=1.0, wd=5e-5, mu=0.9)
    for shifts, at in (((0, 0, 0), 0), ((1, 1, 1), N - 1), ((0, 1, 2), 7000)):
        h = gc.HostGuard(gc.synthetic(), shifts=shifts)
        g, w0, m0 = gc.normals(N, 35), gc.normals(N, 36), gc.normals(N, 37, 0.1)
        g[at] = value
        assert guard_ref.skips(g)
        h.load(w0, g, m0)
        h.measure(1.0)
        h.apply(a)
        assert _bytes_equal(h.w, w0) and _bytes_equal(h.m, m0) and _bytes_equal(h.g, g) and h.guards_intact()
        assert h.words() == (1, 1, 1)


def test_counters_over_good_bad_bad_good():
    _lib()
    a = dict(first=0, gs=1.0, wd=5e-5, mu=0.9)
    h = gc.HostGuard(gc.synthetic(), R=2)                # the ring wraps: the decision is read from slot (step - 1) mod R
    good, bad = gc.normals(N, 45), gc.normals(N, 46)
    bad[1234] = np.nan
    w, m = gc.normals(N, 47), gc.normals(N, 48, 0.1)
    h.load(w, None, m)
    ref = guard_ref.Counters()
    seen = []
    for g in (good, bad, bad, good):
        before = (h.w.copy(), h.m.copy())
        h.step(g, a, max_norm=1.0)
        skip = guard_ref.skips(g)
        assert h.words() == ref.step(skip)
        seen.append(h.words())
        if skip:
            assert _bytes_equal(h.w, before[0]) and _bytes_equal(h.m, before[1])
        else:
            w1, m1 = guard_ref.apply_rule(before[0], g, before[1], h.coef(), gc.LR, a["mu"], a["wd"], a["gs"], 0)
            assert _bytes_equal(h.w, w1) and _bytes_equal(h.m, m1)
    assert [s[0] for s in seen] == [0, 1, 1, 0]          # S_SKIP after each step
    assert [s[2] for s in seen] == [0, 1, 2, 0] and [s[1] for s in seen] == [0, 1, 2, 2]
    assert int(h.state[_steplib.S_STEP]) == 4 and int(h.state[_steplib.S_BAD_STEP]) == 1


# -- measure is observe without the scale launch -------------------------------------------------------------------------
@pytest.mark.parametrize("max_norm", [0.0, 10.0, 1e30])
def test_measure_then_the_librarys_scale_gives_the_bytes_of_observe(max_norm):
    _lib()
    off = gc.synthetic()
    g = gc.normals(N, 55)
    obs, mea = gc.HostGuard(off), gc.HostGuard(off)
    obs.load(g=g)
    stepops.observe_host(obs.g, obs.t, obs.ws, obs.state, obs.ring, obs.R, max_norm, 0.5)
    mea.load(g=g)
    mea.measure(max_norm, 0.5)
    assert _bytes_equal(mea.g, g)                        # measure only reads
    assert _bytes_equal(mea.state, obs.state) and _bytes_equal(mea.ring, obs.ring) and _bytes_equal(mea.ws, obs.ws)
    # the library's own multiply: an update with w = -0, no decay, first, grad_scale 1 leaves m = g * coef (or g)
    mea.load(w=np.full(N, -0.0, np.float32))
    mea.apply(dict(first=1, gs=1.0, wd=0.0, mu=0.0))
    assert _bytes_equal(mea.m, obs.g)
    assert (max_norm == 10.0) == (not _bytes_equal(obs.g, g))


# -- refusals -----------------------------------------------------------------------------------------------------------------
def test_apply_refuses_what_it_cannot_run():
    h = _lib()
    g = gc.HostGuard(step_ref.seg_off_of([5, 70]))
    g.load(gc.normals(75, 1), gc.normals(75, 2), gc.normals(75, 3))
    a = dict(first=0, gs=1.0, wd=0.0, mu=0.9)
    before = (g.w.copy(), g.m.copy(), g.state.copy())
    with pytest.raises(Exception, match="nothing has been measured"):
        g.apply(a)                                       # the step counter is 0
    g.measure()
    P = lambda x: x.ctypes.data                          # noqa: E731
    args = lambda **kw: [kw.get("w", P(g.w)), kw.get("g", P(g.g)), kw.get("m", P(g.m)), kw.get("n", 75),  # noqa: E731
                         kw.get("state", P(g.state)), kw.get("ring", P(g.ring)), kw.get("R", g.R), kw.get("S", 2),
                         0.05, 0.9, 0.0, 1.0, 0]
    state1 = g.state.copy()
    for kw in (dict(w=0), dict(g=0), dict(m=0), dict(state=0), dict(ring=0), dict(n=0), dict(n=-1), dict(R=0), dict(S=0),
               dict(w=P(g.w) + 2), dict(m=P(g.w))):
        assert h.x3dstep_apply_host(*args(**kw)) == -1, kw
        assert h.x3dstep_last_error()
    assert _bytes_equal(g.w, before[0]) and _bytes_equal(g.m, before[1]) and _bytes_equal(g.state, state1)
    assert h.x3dstep_apply_host(*args()) == 0


# -- keep -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stagger", [False, True], ids=["aligned", "staggered"])
@pytest.mark.parametrize("skip_word", [0, 1])
def test_keep_twin_saves_and_restores(stagger, skip_word):
    _lib()
    k = gc.HostKeep(stagger=stagger, seed=60)
    assert k.kt.nitems == 4 + 2 and k.kt.snap_n == 4 + 4 + 64 + 68 + 2052 and all(o % 4 == 0 for o in k.offsets())
    old = [b.copy() for b in k.live]
    k.keep(_steplib.KEEP_SAVE)
    live, snap = guard_ref.keep_rule(old, np.zeros(k.kt.snap_n, np.float32), k.offsets(), 0, 0)
    assert _bytes_equal(k.kt.snap, snap) and k.guards_intact()      # the padding of the snapshot stays 0
    new = [gc.normals(b.size, 70 + i) for i, b in enumerate(k.live)]
    for b, v in zip(k.live, new):
        b[:] = v
    k.state[_steplib.S_SKIP] = skip_word
    k.keep(_steplib.KEEP_RESTORE)
    want, snap2 = guard_ref.keep_rule(new, snap, k.offsets(), 1, skip_word)
    for b, v, o, fresh in zip(k.live, want, old, new):
        assert _bytes_equal(b, v) and _bytes_equal(b, o if skip_word == 1 else fresh)
    assert _bytes_equal(k.kt.snap, snap2) and k.guards_intact()
    k.state[_steplib.S_SKIP] = 2                         # only the value 1 restores
    for b, v in zip(k.live, new):
        b[:] = v
    k.keep(_steplib.KEEP_RESTORE)
    assert all(_bytes_equal(b, v) for b, v in zip(k.live, new))


def test_keep_refuses_a_bad_table():
    h = _lib()
    k = gc.HostKeep(seed=80)
    P = lambda x: x.ctypes.data                          # noqa: E731

    def call(table=None, mode=0, **kw):
        t = k.kt.table if table is None else table
        return h.x3dstep_keep_host(kw.get("table_ptr", P(t)), kw.get("nbuf", k.kt.nbuf), kw.get("items", P(k.kt.items)),
                                   kw.get("nitems", k.kt.nitems), kw.get("snap", P(k.kt.snap)),
                                   kw.get("snap_n", k.kt.snap_n), kw.get("state", P(k.state)), mode)

    bad = []
    for field, value in (("addr", 0), ("addr", int(k.kt.table["addr"][2]) + 1), ("offset", k.kt.snap_n - 3),
                         ("offset", -4), ("len", 0)):
        t = k.kt.table.copy()
        t[field][2] = value
        bad.append(dict(table=t))
    short = k.kt.table.copy()
    short["len"][4] = 2048                                # the second item of the last buffer now lies past its end...
    assert call(table=short) == 0                         # ...which is padding, not an error
    over = k.kt.table.copy()
    over["offset"][1] = 0                                 # over the buffer before it
    bad.append(dict(table=over))
    bad += [dict(table_ptr=0), dict(items=0), dict(snap=0), dict(state=0), dict(nbuf=0), dict(nitems=0), dict(snap_n=0),
            dict(snap_n=k.kt.snap_n - 1), dict(mode=2), dict(mode=-1)]
    k.kt.snap[:] = 0
    for kw in bad:
        assert call(**kw) == -1, list(kw)
        assert h.x3dstep_last_error()
    assert not k.kt.snap.any() and k.guards_intact()      # a refused call writes nothing
    assert call() == 0 and k.kt.snap.any()
    with pytest.raises(ValueError):
        stepops.KeepTable([])
    with pytest.raises(ValueError):
        stepops.KeepTable([np.zeros(4, np.float64)])


# -- the same lists under the sanitisers ----------------------------------------------------------------------------------
def _write_apply_case(f, off, R, shifts, steps, seed):
    """One case of tests/guard_check.cpp's file, with what the in-process twin gave as the expectation."""
    h = gc.HostGuard(off, R=R, shifts=shifts)
    n = h.t.n
    w0, m0 = gc.normals(n, seed), gc.normals(n, seed + 1, 0.1)
    h.load(w0, None, m0)
    f.write(struct.pack("<IIIIII", h.t.S, R, len(steps), *shifts))
    f.write(np.asarray(off, "<i8").tobytes())
    f.write(w0.astype("<f4").tobytes() + m0.astype("<f4").tobytes())
    for g, max_norm, a in steps:
        h.step(g, a, max_norm=max_norm)
        f.write(struct.pack("<ddffffI", max_norm, 1.0, gc.LR, a["mu"], a["wd"], a["gs"], a["first"]))
        f.write(g.astype("<f4").tobytes() + h.w.astype("<f4").tobytes() + h.m.astype("<f4").tobytes())
    f.write(h.state.astype("<i8").tobytes())


def _write_keep_case(f, lengths, stagger, skip_word, seed):
    k = gc.HostKeep(lengths, stagger=stagger, seed=seed)
    f.write(struct.pack("<III", len(lengths), 1 if stagger else 0, skip_word))
    f.write(np.asarray(lengths, "<i4").tobytes())
    for b in k.live:
        f.write(b.astype("<f4").tobytes())
    k.keep(_steplib.KEEP_SAVE)
    f.write(k.kt.snap.astype("<f4").tobytes())
    for i, b in enumerate(k.live):
        b[:] = gc.normals(b.size, seed + 100 + i)
        f.write(b.astype("<f4").tobytes())
    k.state[_steplib.S_SKIP] = skip_word
    k.keep(_steplib.KEEP_RESTORE)
    for b in k.live:
        f.write(b.astype("<f4").tobytes())


def test_the_same_lists_in_a_sanitised_stand_alone_program(tmp_path):
    """step_host.cpp and step_core.h compiled with -fsanitize=address,undefined into a program of their own
    (tests/guard_check.cpp), run as a child process on lists of this file, every buffer a heap block of exactly the size
    the library is told; nothing sanitised is loaded into this interpreter."""
    step_program.compiler()
    _lib()
    syn = gc.synthetic()
    good, bad = gc.normals(N, 91), gc.normals(N, 92)
    bad[int(syn[9]) + 7] = np.nan
    inf = good.copy()
    inf[N - 1] = -np.inf
    a0, a1 = gc.ARITH[0], dict(first=0, gs=0.5, wd=5e-5, mu=0.9)
    first = dict(a1, first=1)
    apply_cases = [(syn, 2, (0, 0, 0), [(good, 0.0, first), (bad, 1.0, a1), (inf, 1.0, a1), (good, 10.0, a1)], 200),
                   (syn, 3, (1, 1, 1), [(gc.eights(N, 93), 512.0, a1), (good, 10.0, a1)], 210),
                   (syn, 3, (3, 3, 3), [(good, 10.0, a0)], 220),
                   (syn, 3, (0, 1, 2), [(good, 10.0, a1), (bad, 10.0, a1)], 230)]
    for n in step_ref.EDGE_LENGTHS:
        apply_cases.append((step_ref.seg_off_of([n]), 1, (n % 4,) * 3, [(gc.normals(n, 94), 0.5, a1)], 240 + n))
    keep_cases = [(gc.KEEP_LENGTHS, True, 1, 300), (gc.KEEP_LENGTHS, False, 0, 310), ([1], True, 1, 320),
                  ([2048, 2049, 4097, 7], True, 1, 330)]
    path = str(tmp_path / "guard_cases.bin")
    with open(path, "wb") as f:
        f.write(struct.pack("<II", len(apply_cases), len(keep_cases)))
        for c in apply_cases:
            _write_apply_case(f, *c)
        for c in keep_cases:
            _write_keep_case(f, *c)
    last, out = step_program.run(tmp_path, "guard_check", path)
    assert last[:2] == ["apply", str(len(apply_cases))] and last[2:4] == ["keep", str(len(keep_cases))], out[-500:]
    assert int(last[-1]) == 0, out[-500:]
