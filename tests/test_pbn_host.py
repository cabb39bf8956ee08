"""Precise BN statistics of libx3dstep on the host: x3dstep_pbn_accum_host and x3dstep_pbn_finish_host (the code of the kernels
through step_core.h) against the numpy restatement tests/pbn_ref.py, byte for byte and inside guard bands; the Fraction bound
of the rule itself; the exact cases; the NaN rule; the refusals; the ABI; the same lists in a sanitised stand-alone program.
No GPU."""
import os
import re
import struct
import subprocess

import numpy as np
import pytest

from tests import guard_cases as gc
from tests import pbn_cases as pc
from tests import pbn_ref
from tests import step_program
from x3dhip import _steplib, stepops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("x3dstep_pbn_layer_bytes", "x3dstep_pbn_build_layers", "x3dstep_pbn_work_count", "x3dstep_pbn_build_work",
       "x3dstep_pbn_accum", "x3dstep_pbn_accum_host", "x3dstep_pbn_finish", "x3dstep_pbn_finish_host")


def _lib():
    if not os.path.exists(_steplib.LIB_PATH):
        import __graft_entry__ as ge
        ge.build()
    return _steplib.lib()


def _bytes_equal(a, b):
    return np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


# -- ABI --------------------------------------------------------------------------------------------------------------------
def test_the_new_entry_points_are_exported_and_bound_and_the_abi_is_still_1():
    h = _lib()
    src = open(os.path.join(ROOT, "include", "x3dstep.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    out = subprocess.run(["nm", "-D", "--defined-only", _steplib.LIB_PATH], capture_output=True, text=True).stdout
    exported = set(re.findall(r"\bT (x3dstep_[a-z0-9_]+)", out))
    for name in NEW:
        assert name in _steplib.SIGNATURES and hasattr(h, name) and name in exported
        decl = re.search(r"\b%s\s*\(([^)]*)\)" % name, code).group(1)
        nargs = 0 if decl.strip() == "void" else len(decl.split(","))
        assert nargs == len(_steplib.SIGNATURES[name][1]), name
    assert h.x3dstep_abi_version() == 1 == _steplib.ABI_VERSION
    assert h.x3dstep_pbn_layer_bytes() == 48 == _steplib.PBN_LAYER_DT.itemsize
    assert h.x3dstep_item_bytes() == 16 and h.x3dstep_keep_bytes() == 24 and h.x3dstep_header_bytes() == 40
    for name, val in (("PBN_RUN", _steplib.PBN_RUN), ("PBN_ACC_DOUBLES", _steplib.PBN_ACC_DOUBLES)):
        assert int(re.search(r"#define X3DSTEP_%s (\d+)" % name, src).group(1)) == val
    for f in ("pbn_accum", "pbn_accum_host", "pbn_finish", "pbn_finish_host", "PbnTable"):
        assert callable(getattr(stepops, f))


def test_the_work_table_cuts_layers_into_runs_of_at_most_256_channels():
    _lib()
    h = pc.HostPbn(pc.grid_shapes(2))
    pt = h.pt
    assert pt.channels == sum(pc.CHANNELS) and pt.nlayers == len(pc.CHANNELS)
    assert list(pt.layers["first"]) == list(np.cumsum([0] + pc.CHANNELS[:-1]))
    assert list(pt.layers["C"]) == pc.CHANNELS and set(pt.layers["S"]) == {2}
    assert list(pt.layers["mean_off"]) == h.offsets()[0::2] and list(pt.layers["var_off"]) == h.offsets()[1::2]
    want = []
    for l, C in enumerate(pc.CHANNELS):
        want += [(int(pt.layers["first"][l]) + at, l, min(256, C - at)) for at in range(0, C, 256)]
    assert [(int(w["start"]), int(w["seg"]), int(w["len"])) for w in pt.work] == want
    assert pt.nwork == len(pc.CHANNELS) + 2                      # 257 and 432 take two runs


# -- the bound of the rule itself, before anything is held to it ----------------------------------------------------------------
def test_the_rule_is_within_one_ulp_of_the_exact_pooled_value_on_every_list_the_tests_use():
    """Every list the grid below feeds a channel is a prefix of one column of pc.POOL (cell i is row i), cut into ranks by
    rank_batches.  For each kind, column, S, K and W: the restatement's fp32 results lie within one fp32 ulp of the exact
    rational mean and variance rounded once.  (fp64 carries 29 bits more than fp32; the streaming update loses a few ulp
    of fp64 per cell, far below half an fp32 ulp, so the fp32 rounding of the rule's fp64 value can differ from the rounding
    of the exact value by at most one step.)"""
    worst = 0
    for kind in pc.KINDS:
        mu, v = pc.POOL[kind]
        for S in pc.SPLITS:
            for K in pc.BATCHES:
                for W in pc.RANKS:
                    counts = [kb * S for kb in pc.rank_batches(K, W)]
                    n = sum(counts)
                    ranks, at = [], 0
                    for cnt in counts:
                        ranks.append([(mu[i], v[i]) for i in range(at, at + cnt)])
                        at += cnt
                    m32, v32 = pbn_ref.pooled(ranks, n)
                    for col in range(pc.COLUMNS):
                        em, ev = pbn_ref.exact_pooled(mu[:n, col], v[:n, col])
                        dm = pbn_ref.ulps32(m32[col], pbn_ref.round32(em))
                        dv = pbn_ref.ulps32(v32[col], pbn_ref.round32(ev))
                        worst = max(worst, dm, dv)
                        assert dm <= 1 and dv <= 1, (kind, S, K, W, col, dm, dv)
    assert worst <= 1


def test_the_hard_list_is_hard():
    """Means 1000 +- 1e-3 with variances near 1e-6: the one-pass E[x^2] - E[x]^2 in fp32 would lose everything; the
    between-cell term is of the size of the within-cell one."""
    mu, v = pc.POOL["hard"]
    assert np.all(np.abs(mu - 1000) <= 1.1e-3) and np.all((v > 4e-7) & (v < 1.6e-6))
    em, ev = pbn_ref.exact_pooled(mu[:40, 0], v[:40, 0])
    within = sum(float(x) for x in v[:40, 0]) / 40
    assert 0.1 < (float(ev) - within) / within < 10


# -- the twin against the restatement ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", pc.SPLITS)
@pytest.mark.parametrize("rot", [0, 1, 2, 3])
def test_the_twin_equals_the_restatement(S, rot):
    """Every C of the grid as a layer of one table, every K and W, both kinds of lists, the buffers at every residue mod 4
    over the four rotations; the live buffers are only read, the padding of the snapshot and every guard band stay."""
    _lib()
    h = pc.HostPbn(pc.grid_shapes(S), rot=rot)
    assert {b.ctypes.data % 16 for b in h.live} == {0, 4, 8, 12}
    for kind in pc.KINDS:
        for K in pc.BATCHES:
            for W in pc.RANKS:
                acc_all, cells, per_layer = h.run(kind, K, W)
                live0 = [b.copy() for b in h.live]
                h.snap[:] = h.SNAP_FILL
                before = h.snap.copy()
                stepops.pbn_finish_host(h.pt, acc_all, W, cells, h.snap)
                want = h.expected_snap(per_layer, cells, before)
                assert _bytes_equal(h.snap, want), (kind, K, W)
                assert not np.any(np.isnan(h.snap)) and h.guards_intact()
                assert all(_bytes_equal(b, b0) for b, b0 in zip(h.live, live0))
                touched = h.snap != before
                assert int(touched.sum()) == 2 * S * sum(pc.CHANNELS)          # nothing outside the S * C elements
                # the accumulators: the restatement's, byte for byte
                for r in range(W):
                    mine = acc_all.reshape(W, -1, 4)[r]
                    for l, (C, _) in enumerate(h.shapes):
                        a = pbn_ref.new_acc(C)
                        for mu, v in per_layer[l][r]:
                            pbn_ref.cell_rule(a, mu, v)
                        f = int(h.pt.layers["first"][l])
                        assert _bytes_equal(mine[f:f + C], a), (kind, K, W, r, l)


# -- exact cases ------------------------------------------------------------------------------------------------------------------
def test_one_cell_returns_the_cell_and_identical_batches_return_the_cell():
    _lib()
    for kind in pc.KINDS:
        h = pc.HostPbn([(65, 1), (257, 1)])
        acc = h.pt.new_acc()
        h.load_batch(kind, 3)
        live0 = [b.copy() for b in h.live]
        stepops.pbn_accum_host(h.pt, acc)
        stepops.pbn_finish_host(h.pt, acc, 1, 1, h.snap)
        for b, off in zip(live0, h.offsets()):
            assert _bytes_equal(h.snap[off:off + b.size], b)
        for K in (2, 5, 7):                                   # K identical batches, S = 1: d = 0 from the second on
            acc[:] = 0
            h.snap[:] = h.SNAP_FILL
            for _ in range(K):
                stepops.pbn_accum_host(h.pt, acc)
            stepops.pbn_finish_host(h.pt, acc, 1, K, h.snap)
            # the mean: d = 0 after the first cell.  The variance: (v + .. + v) / K; an fp32 value times K <= 7 is exact
            # in fp64 at every step of the sum, and the quotient is v again
            for b, off in zip(live0, h.offsets()):
                assert _bytes_equal(h.snap[off:off + b.size], b), (kind, K)
        assert h.guards_intact()


# -- the NaN rule and the special values ------------------------------------------------------------------------------------------
def test_a_count_that_differs_from_expect_n_gives_nan_for_those_channels_only():
    _lib()
    h = pc.HostPbn([(24, 2), (300, 2)])
    acc_all, cells, per_layer = h.run("normal", 2, 1)
    acc = acc_all.reshape(-1, 4)
    odd = [0, 5, 23, 24, 24 + 255, 24 + 256, 24 + 299]          # channels of the accumulator array
    acc[odd, 0] += 1.0
    stepops.pbn_finish_host(h.pt, acc_all, 1, cells, h.snap)
    want = h.expected_snap(per_layer, cells, np.full_like(h.snap, h.SNAP_FILL))
    offs = h.offsets()
    bad = np.zeros(h.snap.size, bool)
    for ch in odd:
        l, c = (0, ch) if ch < 24 else (1, ch - 24)
        C = h.shapes[l][0]
        for j in range(2):
            bad[offs[2 * l] + j * C + c] = bad[offs[2 * l + 1] + j * C + c] = True
    assert np.array_equal(np.isnan(h.snap), bad)
    assert _bytes_equal(h.snap[~bad], want[~bad]) and h.guards_intact()


def test_nan_and_inf_cells_propagate_as_the_arithmetic_gives_them():
    _lib()
    inf, nan = np.inf, np.nan
    mus = np.array([[1.0, nan, inf, -inf, 1.0, 1.0, inf, 2.0], [3.0, 1.0, 1.0, 1.0, 3.0, 3.0, -inf, 2.0]], np.float32)
    vs = np.array([[1.0, 1.0, 1.0, 1.0, nan, inf, 1.0, inf], [1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, -inf]], np.float32)
    h = pc.HostPbn([(8, 2)])
    h.live[0][:], h.live[1][:] = mus.reshape(-1), vs.reshape(-1)
    acc = h.pt.new_acc()
    stepops.pbn_accum_host(h.pt, acc)
    stepops.pbn_finish_host(h.pt, acc, 1, 2, h.snap)
    m32, v32 = pbn_ref.pooled([[(mus[0], vs[0]), (mus[1], vs[1])]], 2)
    offs = h.offsets()
    assert _bytes_equal(h.snap[offs[0]:offs[0] + 8], m32) and _bytes_equal(h.snap[offs[1]:offs[1] + 8], v32)
    gm, gv = h.snap[offs[0]:offs[0] + 8], h.snap[offs[1]:offs[1] + 8]
    assert gm[0] == 2.0 and gv[0] == 2.0                      # (1 + 1) / 2 + ((1 - 2)^2 + (3 - 2)^2) / 2
    assert np.isnan(gm[1]) and np.isnan(gv[1])                # a NaN mean poisons both
    assert np.isnan(gm[2]) and np.isnan(gm[3])                # Inf - Inf inside the streaming mean
    assert gm[4] == 2.0 and np.isnan(gv[4]) and gm[5] == 2.0 and gv[5] == inf
    assert np.isnan(gm[6]) and gm[7] == 2.0 and np.isnan(gv[7])


# -- the refusals -------------------------------------------------------------------------------------------------------------------
def test_every_refusal_is_einval_with_a_message_and_writes_nothing():
    h_ = _lib()
    h = pc.HostPbn([(24, 2), (300, 2), (5, 2)])
    acc_all, cells, _ = h.run("normal", 1, 2)
    acc0, snap0 = acc_all.copy(), h.snap.copy()
    pt = h.pt
    P = lambda x: x.ctypes.data                          # noqa: E731
    keep = []

    def call(finish, **kw):
        layers, work = kw.get("layers", pt.layers), kw.get("work", pt.work)
        keep.extend([layers, work])
        head = [kw.get("layers_ptr", P(layers)), kw.get("nlayers", pt.nlayers), kw.get("work_ptr", P(work)),
                kw.get("nwork", pt.nwork), kw.get("acc", P(acc_all))]
        if not finish:
            return h_.x3dstep_pbn_accum_host(*head)
        return h_.x3dstep_pbn_finish_host(*head, kw.get("W", 2), kw.get("expect_n", cells), kw.get("snap", P(h.snap)),
                                          kw.get("snap_n", pt.snap_n))

    def layers_with(l, field, value):
        t = pt.layers.copy()
        t[field][l] = value
        return dict(layers=t)

    def work_with(i, field, value):
        t = pt.work.copy()
        t[field][i] = value
        return dict(work=t)

    both = [dict(layers_ptr=0), dict(work_ptr=0), dict(acc=0), dict(nlayers=0), dict(nwork=0), dict(nwork=pt.nlayers - 1),
            dict(layers_ptr=P(pt.layers) + 4), dict(acc=P(acc_all) + 4),
            layers_with(1, "mean_addr", 0), layers_with(1, "var_addr", 0),
            layers_with(1, "mean_addr", int(pt.layers["mean_addr"][1]) + 2),
            layers_with(2, "var_addr", int(pt.layers["var_addr"][2]) + 1),
            layers_with(0, "C", 0), layers_with(1, "C", -1), layers_with(1, "S", 0), layers_with(2, "S", -2),
            layers_with(1, "first", 25), layers_with(0, "first", -1), layers_with(1, "C", 299),
            work_with(1, "seg", 0), work_with(1, "seg", 3), work_with(1, "seg", -1), work_with(1, "len", 0),
            work_with(1, "len", 257), work_with(2, "len", 45), work_with(0, "len", 25), work_with(2, "start", 24 + 255),
            work_with(1, "start", 23), work_with(3, "start", 24 + 300 + 1), work_with(0, "start", -1)]
    only_finish = [dict(W=0), dict(W=-1), dict(expect_n=0), dict(snap=0), dict(snap=P(h.snap) + 2), dict(snap_n=0),
                   dict(snap_n=pt.snap_n - 4),
                   layers_with(1, "mean_off", -4), layers_with(2, "var_off", pt.snap_n - 8),
                   layers_with(1, "mean_off", int(pt.layers["mean_off"][1]) - 4),          # over the buffer before it
                   layers_with(1, "var_off", int(pt.layers["var_off"][1]) - 4),            # over its own means
                   layers_with(1, "S", 3)]                                                 # S * C no longer fits
    for kw in both:
        for finish in (False, True):
            assert call(finish, **kw) == -1, (finish, {k: None for k in kw})
            assert h_.x3dstep_last_error()
    for kw in only_finish:
        assert call(True, **kw) == -1, {k: None for k in kw}
        assert h_.x3dstep_last_error()
    assert _bytes_equal(acc_all, acc0) and _bytes_equal(h.snap, snap0) and h.guards_intact()
    with pytest.raises(Exception, match="x3dstep_pbn_finish_host"):
        stepops.pbn_finish_host(pt, acc_all, 2, 0, h.snap)
    with pytest.raises(ValueError):
        stepops.pbn_finish_host(pt, acc_all[:-4], 2, cells, h.snap)
    with pytest.raises(ValueError):
        stepops.pbn_accum_host(pt, acc_all)                  # two ranks' accumulators where one is taken
    with pytest.raises(ValueError):
        stepops.PbnTable(h.kt, [2, 2])
    with pytest.raises(Exception, match="x3dstep_pbn_build_layers"):
        stepops.PbnTable(h.kt, [2, 7, 2])                    # 600 elements are no multiple of 7
    assert call(True) == 0 and not _bytes_equal(h.snap, snap0)
    assert call(False, acc=P(acc_all[:4 * pt.channels])) == 0


# -- the same lists under the sanitisers ------------------------------------------------------------------------------------
def _write_case(f, shapes, rot, kind, K, W, miscount):
    h = pc.HostPbn(shapes, rot=rot)
    batches = pc.rank_batches(K, W)
    S = shapes[0][1]
    f.write(struct.pack("<IIIi", len(shapes), rot, W, miscount))
    f.write(np.asarray([x for cs in shapes for x in cs], "<i4").tobytes())
    f.write(np.asarray(batches, "<i4").tobytes())
    acc_all = h.pt.new_acc(W).reshape(W, -1)
    at = 0
    for r, kb in enumerate(batches):
        acc = h.pt.new_acc()
        for _ in range(kb):
            h.load_batch(kind, at)
            at += S
            for b in h.live:
                f.write(b.astype("<f4").tobytes())
            stepops.pbn_accum_host(h.pt, acc)
        acc_all[r] = acc
    expect_n = at + miscount
    stepops.pbn_finish_host(h.pt, acc_all.reshape(-1), W, expect_n, h.snap)
    f.write(struct.pack("<fq", h.SNAP_FILL, expect_n))
    f.write(acc_all.astype("<f8").tobytes())
    f.write(h.snap.astype("<f4").tobytes())


def test_the_same_lists_in_a_sanitised_stand_alone_program(tmp_path):
    """step_host.cpp and step_core.h compiled with -fsanitize=address,undefined into a program of their own
    (tests/pbn_check.cpp), run as a child process on lists of this file, every buffer a heap block of exactly the size the
    library is told; nothing sanitised is loaded into this interpreter."""
    step_program.compiler()
    _lib()
    cases = []
    for i, S in enumerate(pc.SPLITS):
        for j, W in enumerate(pc.RANKS):
            cases.append((pc.grid_shapes(S), (i + j) % 4, pc.KINDS[(i + j) % 2], pc.BATCHES[(i + j) % 3], W, 0))
    cases += [([(1, 1)], 0, "hard", 1, 1, 0), ([(257, 3), (2, 3)], 3, "normal", 2, 3, 1)]
    path = str(tmp_path / "pbn_cases.bin")
    with open(path, "wb") as f:
        f.write(struct.pack("<I", len(cases)))
        for c in cases:
            _write_case(f, *c)
    last, out = step_program.run(tmp_path, "pbn_check", path)
    assert last[:2] == ["pbn", str(len(cases))] and int(last[-1]) == 0, out[-500:]
