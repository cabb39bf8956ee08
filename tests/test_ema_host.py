"""The weight average of libx3dstep on the host: x3dstep_ema_host, x3dstep_ema_keep_host, x3dstep_swap_host and
x3dstep_swap_keep_host (the code of the kernels through step_core.h) against the numpy restatement tests/ema_ref.py, byte
for byte and inside guard bands; the count, skip and decay rules; the refusals; the ABI; the same lists in a sanitised
stand-alone program.  No GPU."""
import os
import re
import struct

import numpy as np
import pytest

from tests import ema_cases as ec
from tests import ema_ref
from tests import guard_cases as gc
from tests import step_program
from x3dhip import _steplib, stepops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("x3dstep_ema", "x3dstep_ema_host", "x3dstep_ema_keep", "x3dstep_ema_keep_host", "x3dstep_swap", "x3dstep_swap_host",
       "x3dstep_swap_keep", "x3dstep_swap_keep_host")


def _lib():
    if not os.path.exists(_steplib.LIB_PATH):
        import __graft_entry__ as ge
        ge.build()
    return _steplib.lib()


def _bytes_equal(a, b):
    return np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


def _intact(big, shift, n):
    lo, hi = gc.GUARD + shift, gc.GUARD + shift + n
    return bool(np.all(big[:lo] == gc.FILL)) and bool(np.all(big[hi:] == gc.FILL))


# -- ABI --------------------------------------------------------------------------------------------------------------------
def test_the_new_entry_points_are_exported_and_bound_and_the_abi_is_still_1():
    h = _lib()
    src = open(os.path.join(ROOT, "include", "x3dstep.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name in NEW:
        assert name in _steplib.SIGNATURES and hasattr(h, name)
        decl = re.search(r"\b%s\s*\(([^)]*)\)" % name, code).group(1)
        assert len(decl.split(",")) == len(_steplib.SIGNATURES[name][1]), name
    assert h.x3dstep_abi_version() == 1 == _steplib.ABI_VERSION
    assert h.x3dstep_header_bytes() == 40 and _steplib.STATE_WORDS == 8
    assert int(re.search(r"#define X3DSTEP_STATE_WORDS (\d+)", src).group(1)) == 8
    for f in ("ema", "ema_host", "ema_keep", "ema_keep_host", "swap", "swap_host", "swap_keep", "swap_keep_host"):
        assert callable(getattr(stepops, f))


# -- the rules of the restatement ---------------------------------------------------------------------------------------------
def test_the_count_and_decay_rules():
    assert ema_ref.count_rule(None, 7) == 7
    st = ec.state_for(12, -7)
    assert ema_ref.count_rule(st, -7) == 12 and not ema_ref.skips(st) and not ema_ref.skips(None)
    assert ema_ref.skips(ec.state_for(3, 0, skip=1)) and not ema_ref.skips(ec.state_for(3, 0, skip=2))
    d99 = float(np.float32(0.9999))
    # both sides of the min: (1 + k) / (10 + k) crosses 0.9999 between k = 89989 and 89991; the fp32 decay lies below both
    assert (1 + 10) / (10.0 + 10) < d99 < (1 + 89989) / (10.0 + 89989) < 0.9999 < (1 + 89991) / (10.0 + 89991)
    assert ema_ref.decay_rule(1, 0.9999, True)[0] == np.float32(2 / 11.0)
    assert ema_ref.decay_rule(9, 0.9, True)[0] == np.float32(10 / 19.0)
    assert ema_ref.decay_rule(10, 0.5, True)[0] == np.float32(0.5)            # 11 / 20 > 0.5
    assert ema_ref.decay_rule(89991, 0.9999, True)[0] == np.float32(0.9999)
    assert ema_ref.decay_rule(1, 0.9999, False) == (np.float32(0.9999), np.float32(1.0 - d99))
    d, omd = ema_ref.decay_rule(2, 0.9, True)
    assert d == np.float32(0.25) and omd == np.float32(0.75)
    assert ema_ref.decay_rule(5, 0.0, True) == (np.float32(0.0), np.float32(1.0))


# -- exact inputs first: where plain fp64 is the answer -------------------------------------------------------------------------
@pytest.mark.parametrize("decay", [0.5, 0.75])
def test_on_integer_inputs_the_twin_equals_plain_fp64(decay):
    """e and w small integers and d a multiple of 1/4: d * e + (1 - d) * w is a multiple of 1/4 below 2^12, exact in fp32
    whatever the order and the number of roundings -- shown first, then demanded of the restatement and of the twin."""
    _lib()
    rng = np.random.default_rng(11)
    n = 4097
    e0 = rng.integers(-1000, 1001, n).astype(np.float32)
    w = rng.integers(-1000, 1001, n).astype(np.float32)
    plain = decay * e0.astype(np.float64) + (1.0 - decay) * w.astype(np.float64)
    assert np.array_equal(plain * 4, np.round(plain * 4)) and np.abs(plain).max() <= 1000      # exact, on fp32's grid
    assert np.array_equal(plain.astype(np.float32).astype(np.float64), plain)
    d, omd = ema_ref.decay_rule(1, decay, False)
    assert float(d) == decay and float(omd) == 1.0 - decay
    assert np.array_equal(ema_ref.element_rule(e0, w, d, omd).astype(np.float64), plain)
    for se, sw in ec.SHIFTS:
        (ebig, e), (wbig, wv) = gc.banded(n, se), gc.banded(n, sw)
        e[:], wv[:] = e0, w
        stepops.ema_host(e, wv, None, 1, decay, warmup=False)
        assert np.array_equal(e.astype(np.float64), plain) and _bytes_equal(wv, w)
        assert _intact(ebig, se, n) and _intact(wbig, sw, n)


# -- the twin against the restatement -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", ec.LENGTHS)
def test_ema_twin_equals_the_restatement(n):
    _lib()
    e0, w = gc.normals(n, 100 + n), gc.normals(n, 200 + n, 0.5)
    moved = 0
    for (se, sw) in ec.SHIFTS:
        (ebig, e), (wbig, wv) = gc.banded(n, se), gc.banded(n, sw)
        wv[:] = w
        for decay in ec.DECAYS:
            for warmup in (True, False):
                for k in ec.KS:
                    d, omd = ema_ref.decay_rule(k, decay, warmup)
                    want = ema_ref.element_rule(e0, w, d, omd)
                    for with_state in (False, True):
                        for state, count in ec.counts(k, with_state):
                            e[:] = e0
                            before = None if state is None else state.copy()
                            stepops.ema_host(e, wv, state, count, decay, warmup)
                            assert _bytes_equal(e, want), (se, sw, decay, warmup, k, count)
                            assert _bytes_equal(wv, w) and _intact(ebig, se, n) and _intact(wbig, sw, n)
                            assert state is None or _bytes_equal(state, before)          # the state is only read
                            assert _bytes_equal(want, ema_ref.update(e0, w, state, count, decay, warmup))
                    moved += int(not _bytes_equal(want, e0))
    assert moved > 0


def test_a_skip_word_of_1_leaves_every_byte_alone():
    _lib()
    n = 4097
    e0, w = gc.normals(n, 1), gc.normals(n, 2)
    for se, sw in ec.SHIFTS:
        (ebig, e), (wbig, wv) = gc.banded(n, se), gc.banded(n, sw)
        e[:], wv[:] = e0, w
        st = ec.state_for(4, 0, skip=1)
        assert ema_ref.update(e0, w, st, 0, 0.9, True) is None
        stepops.ema_host(e, wv, st, 0, 0.9, True)
        assert _bytes_equal(e, e0) and _bytes_equal(wv, w) and _intact(ebig, se, n) and _intact(wbig, sw, n)
        st[_steplib.S_SKIP] = 2                          # only the value 1 skips
        stepops.ema_host(e, wv, st, 0, 0.9, True)
        assert not _bytes_equal(e, e0)
    k = ec.HostEmaKeep(seed=5)
    before = k.esnap.copy()
    stepops.ema_keep_host(k.kt, k.esnap, ec.state_for(4, 0, skip=1), 0, 0.9, True)
    assert _bytes_equal(k.esnap, before) and k.guards_intact()


def test_nan_inf_and_negative_zero_propagate_as_the_arithmetic_gives_them():
    _lib()
    inf, nan = np.inf, np.nan
    e0 = np.array([nan, 1.0, inf, inf, -inf, 1.0, -0.0, -0.0, 0.0, 2.0, inf, 3.0], np.float32)
    w = np.array([1.0, nan, 1.0, -inf, -inf, inf, -0.0, 0.0, -0.0, -inf, inf, -0.0], np.float32)
    for decay, want in ((0.5, [nan, nan, inf, nan, -inf, inf, -0.0, 0.0, 0.0, -inf, inf, 1.5]),
                        (0.0, [nan, nan, nan, nan, nan, inf, -0.0, 0.0, 0.0, -inf, nan, 0.0])):
        # decay 0: d = +0 and 0 * Inf is a NaN; d * -0 = -0 and -0 + -0 = -0, every other sum of zeros +0
        for shift in (0, 1):
            (_, e), (_, wv) = gc.banded(e0.size, shift), gc.banded(e0.size, shift)
            e[:], wv[:] = e0, w
            stepops.ema_host(e, wv, None, 1, decay, warmup=False)
            want = np.array(want, np.float32)
            assert np.array_equal(np.isnan(e), np.isnan(want)), (decay, e)
            ok = ~np.isnan(want)
            assert np.array_equal(e[ok], want[ok]) and np.array_equal(np.signbit(e[ok]), np.signbit(want[ok])), (decay, e)


def test_ema_refuses_what_it_cannot_run():
    h = _lib()
    n = 70
    (_, e), (_, w) = gc.banded(n, 0), gc.banded(n, 0)
    e[:], w[:] = gc.normals(n, 1), gc.normals(n, 2)
    before = e.copy()
    st = ec.state_for(3, 0)
    P = lambda x: x.ctypes.data                          # noqa: E731
    args = lambda **kw: [kw.get("e", P(e)), kw.get("w", P(w)), kw.get("n", n), kw.get("state", P(st)),  # noqa: E731
                         kw.get("count", 0), kw.get("decay", 0.9), 1]
    for kw in (dict(e=0), dict(w=0), dict(n=0), dict(n=-1), dict(e=P(e) + 2), dict(w=P(w) + 1), dict(state=P(st) + 4),
               dict(decay=1.0), dict(decay=-0.1), dict(decay=float("nan")), dict(decay=1.5), dict(w=P(e)), dict(w=P(e) + 4 * (n - 1)),
               dict(count=-3), dict(count=-4), dict(state=None, count=0), dict(state=None, count=-1)):
        assert h.x3dstep_ema_host(*args(**kw)) == -1, kw
        assert h.x3dstep_last_error()
    assert _bytes_equal(e, before)
    with pytest.raises(Exception, match="nothing to average"):
        stepops.ema_host(e, w, st, -3, 0.9)
    assert h.x3dstep_ema_host(*args(state=None, count=1)) == 0 and h.x3dstep_ema_host(*args(count=-2)) == 0
    a, b = gc.banded(n, 0)[1], gc.banded(n, 1)[1]
    for call in ((0, P(b), n), (P(a), 0, n), (P(a), P(b), 0), (P(a) + 1, P(b), n), (P(a), P(a), n), (P(a), P(a) + 8, n)):
        assert h.x3dstep_swap_host(*call) == -1 and h.x3dstep_last_error()
    assert h.x3dstep_swap_host(P(a), P(a) + 4 * (n // 2), n // 2) == 0          # adjacent, not overlapping


# -- the keep-table form --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rot", [0, 1, 2, 3])
def test_ema_keep_twin_equals_the_restatement(rot):
    """Every buffer length at every start residue mod 4 over the four rotations; the padding of the averaged snapshot and
    everything around it stay as they were."""
    _lib()
    k = ec.HostEmaKeep(rot=rot, seed=10 * rot)
    assert {b.ctypes.data % 16 for b in k.live} == {0, 4, 8, 12} and all(o % 4 == 0 for o in k.offsets())
    for decay, warmup, kk, with_state in ((0.9, True, 1, True), (0.9, True, 10, False), (0.9999, True, 89991, True),
                                          (0.5, False, 2, True), (0.0, False, 9, False), (0.9999, False, 1, True)):
        for state, count in ec.counts(kk, with_state):
            live0 = [b.copy() for b in k.live]
            k.esnap[:] = gc.normals(k.kt.snap_n, 33 + count)
            snap0 = k.esnap.copy()
            stepops.ema_keep_host(k.kt, k.esnap, state, count, decay, warmup)
            d, omd = ema_ref.decay_rule(kk, decay, warmup)
            want = snap0.copy()
            for b, off in zip(live0, k.offsets()):
                want[off:off + b.size] = ema_ref.element_rule(snap0[off:off + b.size], b, d, omd)
            assert _bytes_equal(k.esnap, want) and k.guards_intact()
            assert all(_bytes_equal(b, v) for b, v in zip(k.live, live0))
            assert not _bytes_equal(want, snap0)


def test_the_table_forms_refuse_a_bad_table():
    h = _lib()
    k = ec.HostEmaKeep(lengths=gc.KEEP_LENGTHS, seed=80)
    st = ec.state_for(2, 0)
    P = lambda x: x.ctypes.data                          # noqa: E731

    def call(swap, table=None, **kw):
        t = k.kt.table if table is None else table
        head = [kw.get("table_ptr", P(t)), kw.get("nbuf", k.kt.nbuf), kw.get("items", P(k.kt.items)),
                kw.get("nitems", k.kt.nitems), kw.get("snap", P(k.esnap)), kw.get("snap_n", k.kt.snap_n)]
        if swap:
            return h.x3dstep_swap_keep_host(*head)
        return h.x3dstep_ema_keep_host(*head, kw.get("state", P(st)), kw.get("count", 0), kw.get("decay", 0.9), 1)

    bad = []
    for field, value in (("addr", 0), ("addr", int(k.kt.table["addr"][2]) + 1), ("offset", k.kt.snap_n - 3), ("offset", -4),
                         ("len", 0)):
        t = k.kt.table.copy()
        t[field][2] = value
        bad.append(dict(table=t))
    over = k.kt.table.copy()
    over["offset"][1] = 0
    bad.append(dict(table=over))
    bad += [dict(table_ptr=0), dict(items=0), dict(snap=0), dict(nbuf=0), dict(nitems=0), dict(snap_n=0),
            dict(snap_n=k.kt.snap_n - 1)]
    for field, value in (("seg", k.kt.nbuf), ("seg", -1), ("len", 0), ("len", 2049), ("start", -1), ("start", k.kt.snap_n)):
        it = k.kt.items.copy()                           # the per-item tests: the twin refuses the call for one bad item
        it[field][1] = value
        bad.append(dict(items=P(it), keepalive=it))
    before, live0 = k.esnap.copy(), [b.copy() for b in k.live]
    for kw in bad:
        for swap in (False, True):
            assert call(swap, **kw) == -1, (swap, list(kw))
            assert h.x3dstep_last_error()
    for kw in (dict(decay=1.0), dict(decay=float("nan")), dict(count=-2), dict(state=None, count=0), dict(state=P(st) + 4)):
        assert call(False, **kw) == -1, list(kw)
        assert h.x3dstep_last_error()
    assert _bytes_equal(k.esnap, before) and all(_bytes_equal(b, v) for b, v in zip(k.live, live0)) and k.guards_intact()
    assert call(False) == 0 and not _bytes_equal(k.esnap, before)
    assert call(False, state=None, count=1) == 0


# -- the exchange ---------------------------------------------------------------------------------------------------------------
def _bit_patterns(n, seed):
    """Random 32-bit patterns -- NaNs with payloads, infinities, subnormals, both zeros among them -- as float32."""
    bits = np.random.default_rng(seed).integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32)
    special = np.array([0x7fc00001, 0xffc12345, 0x7f800001, 0xff8fffff, 0x7f800000, 0xff800000, 0x80000000, 0, 1, 0x80000001],
                       np.uint32)
    m = min(n, special.size)
    bits[:m] = special[:m]
    return bits.view(np.float32)


@pytest.mark.parametrize("n", ec.LENGTHS)
def test_swap_twin_exchanges_bits_and_twice_is_the_identity(n):
    _lib()
    a0, b0 = _bit_patterns(n, n), _bit_patterns(n, 5000 + n)[::-1].copy()
    for sa, sb in ec.SHIFTS:
        (abig, a), (bbig, b) = gc.banded(n, sa), gc.banded(n, sb)
        a[:], b[:] = a0, b0
        assert _bytes_equal(a, a0)                       # the copy into the band kept the payloads
        stepops.swap_host(a, b)
        assert _bytes_equal(a, b0) and _bytes_equal(b, a0) and _intact(abig, sa, n) and _intact(bbig, sb, n)
        stepops.swap_host(a, b)
        assert _bytes_equal(a, a0) and _bytes_equal(b, b0) and _intact(abig, sa, n) and _intact(bbig, sb, n)


@pytest.mark.parametrize("rot", [0, 1, 2, 3])
def test_swap_keep_twin_exchanges_live_and_snapshot(rot):
    _lib()
    k = ec.HostEmaKeep(rot=rot, seed=7)
    for i, b in enumerate(k.live):
        b[:] = _bit_patterns(b.size, 300 + i)
    k.esnap[:] = _bit_patterns(k.kt.snap_n, 400)
    live0, snap0 = [b.copy() for b in k.live], k.esnap.copy()
    stepops.swap_keep_host(k.kt, k.esnap)
    want = snap0.copy()
    for b, v, off in zip(k.live, live0, k.offsets()):
        assert _bytes_equal(b, snap0[off:off + b.size])
        want[off:off + v.size] = v
    assert _bytes_equal(k.esnap, want) and k.guards_intact()       # the padding of the snapshot is not exchanged
    stepops.swap_keep_host(k.kt, k.esnap)
    assert _bytes_equal(k.esnap, snap0) and all(_bytes_equal(b, v) for b, v in zip(k.live, live0)) and k.guards_intact()


# -- the same lists under the sanitisers ------------------------------------------------------------------------------------
def _write_ema_case(f, n, se, sw, decay, warmup, k, with_state, skip, seed):
    state, count = ec.counts(k, with_state)[-1]
    if state is not None:
        state[_steplib.S_SKIP] = skip
    (_, e), (_, w) = gc.banded(n, se), gc.banded(n, sw)
    e[:], w[:] = gc.normals(n, seed), gc.normals(n, seed + 1)
    f.write(struct.pack("<IIIIIq", n, se, sw, 1 if warmup else 0, 0 if state is None else 1, count))
    f.write((stepops.new_state() if state is None else state).astype("<i8").tobytes())
    f.write(struct.pack("<f", decay))
    f.write(e.astype("<f4").tobytes() + w.astype("<f4").tobytes())
    stepops.ema_host(e, w, state, count, decay, warmup)
    f.write(e.astype("<f4").tobytes())


def _write_keep_case(f, rot, decay, warmup, k, with_state, seed):
    state, count = ec.counts(k, with_state)[-1]
    h = ec.HostEmaKeep(rot=rot, seed=seed)
    f.write(struct.pack("<IIIIq", len(h.lengths), rot, 1 if warmup else 0, 0 if state is None else 1, count))
    f.write((stepops.new_state() if state is None else state).astype("<i8").tobytes())
    f.write(struct.pack("<f", decay))
    f.write(np.asarray(h.lengths, "<i4").tobytes())
    for b in h.live:
        f.write(b.astype("<f4").tobytes())
    f.write(h.esnap.astype("<f4").tobytes())
    stepops.ema_keep_host(h.kt, h.esnap, state, count, decay, warmup)
    f.write(h.esnap.astype("<f4").tobytes())


def test_the_same_lists_in_a_sanitised_stand_alone_program(tmp_path):
    """step_host.cpp and step_core.h compiled with -fsanitize=address,undefined into a program of their own
    (tests/ema_check.cpp), run as a child process on lists of this file, every buffer a heap block of exactly the size the
    library is told; nothing sanitised is loaded into this interpreter."""
    step_program.compiler()
    _lib()
    ema_cases = []
    for i, n in enumerate(ec.LENGTHS):
        se, sw = ec.SHIFTS[i % len(ec.SHIFTS)]
        ema_cases.append((n, se, sw, ec.DECAYS[i % 4], i % 2 == 0, ec.KS[i % 5], i % 3 != 0, 0, 500 + i))
    ema_cases += [(4097, s, s, 0.9999, True, 89991, True, 0, 600 + s) for s in range(4)]
    ema_cases += [(4097, 1, 3, 0.9, True, 2, True, 0, 610), (1025, 2, 2, 0.9, True, 2, True, 1, 611)]
    keep_cases = [(0, 0.9, True, 1, True, 700), (1, 0.9999, True, 89991, False, 710), (2, 0.5, False, 9, True, 720),
                  (3, 0.0, True, 10, True, 730)]
    swap_cases = [(n, sa, sb) for n in ec.LENGTHS for sa, sb in ((n % 4, n % 4), (1, 3))]
    path = str(tmp_path / "ema_cases.bin")
    with open(path, "wb") as f:
        f.write(struct.pack("<III", len(ema_cases), len(keep_cases), len(swap_cases)))
        for c in ema_cases:
            _write_ema_case(f, *c)
        for c in keep_cases:
            _write_keep_case(f, *c)
        for n, sa, sb in swap_cases:
            f.write(struct.pack("<III", n, sa, sb))
            f.write(_bit_patterns(n, n).tobytes() + _bit_patterns(n, 9000 + n).tobytes())
    last, out = step_program.run(tmp_path, "ema_check", path)
    assert last[:6] == ["ema", str(len(ema_cases)), "keep", str(len(keep_cases)), "swap", str(len(swap_cases))], out[-500:]
    assert int(last[-1]) == 0, out[-500:]
