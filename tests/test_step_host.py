"""libx3dstep on the host: the ABI, the item-table builder and the CPU twin (x3dstep_observe_host, the code of the kernels
through step_core.h) against the numpy restatement tests/step_ref.py.  No GPU."""
import math
import os
import re
import shutil
import struct
import subprocess

import numpy as np
import pytest

from tests import step_ref
from tests import step_program
from x3dhip import _steplib, stepops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -53


def _lib():
    if not os.path.exists(_steplib.LIB_PATH):
        import __graft_entry__ as ge
        ge.build()
    return _steplib.lib()


def _header_functions():
    src = open(os.path.join(ROOT, "include", "x3dstep.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(x3dstep_[a-z0-9_]+)\s*\(", src)))


class HostMonitor:
    """The twin's buffers for one segment table: exactly the sizes the library asks for."""

    def __init__(self, seg_off, R=4, misalign=0):
        _lib()
        self.t = stepops.StepTables(seg_off)
        self.R = R
        self.state = stepops.new_state()
        self.ws = stepops.aligned_bytes(self.t.workspace_bytes)
        self.ring = stepops.aligned_bytes(R * self.t.record_bytes)
        self.gbuf = stepops.aligned_bytes(4 * (self.t.n + 4)).view(np.float32)[misalign:misalign + self.t.n]

    def step(self, g, max_norm=0.0, inv_world=1.0):
        """-> (header, sumsq, hash, nonfinite, the gradient after the call) of this step"""
        self.gbuf[:] = g
        step = int(self.state[_steplib.S_STEP])
        stepops.observe_host(self.gbuf, self.t, self.ws, self.state, self.ring, self.R, max_norm, inv_world)
        rb = self.t.record_bytes
        slot = step % self.R
        head, sumsq, hsh, nf = stepops.parse_record(self.ring[slot * rb:(slot + 1) * rb], self.t.S)
        assert head["step"] == step and head["nseg"] == self.t.S
        return head, sumsq.copy(), hsh.copy(), nf.copy(), self.gbuf.copy()


def _integers(n, seed, bound=1024):
    return np.random.default_rng(seed).integers(-bound, bound + 1, n).astype(np.float32)


def _normals(n, seed, scale=1.0):
    return (np.random.default_rng(seed).standard_normal(n) * scale).astype(np.float32)


# -- ABI --------------------------------------------------------------------------------------------------------------------
def test_step_header_ctypes_table_and_exports_agree():
    h = _lib()
    assert _header_functions() == sorted(_steplib.SIGNATURES.keys())
    assert h.x3dstep_abi_version() == _steplib.ABI_VERSION == 1
    out = subprocess.run(["nm", "-D", "--defined-only", _steplib.LIB_PATH], capture_output=True, text=True).stdout
    exported = set(re.findall(r"\bT (x3dstep_[a-z0-9_]+)", out))
    assert set(_header_functions()) <= exported
    src = open(os.path.join(ROOT, "include", "x3dstep.h")).read()
    for name, val in (("ITEM", _steplib.ITEM), ("ITEMS_PER_GROUP", _steplib.ITEMS_PER_GROUP),
                      ("STATE_WORDS", _steplib.STATE_WORDS), ("S_STEP", _steplib.S_STEP), ("S_BAD_STEP", _steplib.S_BAD_STEP),
                      ("S_BAD_SEG", _steplib.S_BAD_SEG), ("S_NORM", _steplib.S_NORM), ("S_COEF", _steplib.S_COEF)):
        assert int(re.search(r"#define X3DSTEP_%s (\d+)" % name, src).group(1)) == val, name
    assert _steplib.ITEM == step_ref.ITEM


def test_step_struct_and_record_sizes():
    h = _lib()
    assert h.x3dstep_item_bytes() == _steplib.ITEM_DT.itemsize == 16
    assert h.x3dstep_header_bytes() == _steplib.HEADER_DT.itemsize == 40
    for S in (1, 2, 3, 12, 316):
        assert h.x3dstep_record_bytes(S) == (40 + 20 * S + 7) // 8 * 8
    assert h.x3dstep_record_bytes(0) == 0 and h.x3dstep_record_bytes(_steplib.MAX_SEGMENTS + 1) == 0
    assert h.x3dstep_workspace_bytes(5) == 104 and h.x3dstep_workspace_bytes(0) == 0
    # the flagship: at least as many workgroups as the card has CUs (256)
    off, _ = step_ref.model_seg_off("M")
    assert h.x3dstep_item_count(off.ctypes.data, len(off) - 1) // _steplib.ITEMS_PER_GROUP >= 256


def test_step_argument_checks():
    h = _lib()
    bad = np.array([0, 4, 4], np.int64)                       # an empty tensor
    assert h.x3dstep_item_count(bad.ctypes.data, 2) == -1 and b"tensor" in h.x3dstep_last_error()
    bad = np.array([1, 4], np.int64)                          # does not start at 0
    assert h.x3dstep_item_count(bad.ctypes.data, 1) == -1
    off = step_ref.seg_off_of([5, 3000])
    items = np.zeros(2, _steplib.ITEM_DT)                     # one item short
    seg_item = np.zeros(3, np.int32)
    assert h.x3dstep_build_items(off.ctypes.data, 2, items.ctypes.data, 2, seg_item.ctypes.data) == -1
    m = HostMonitor(off)
    wrong = m.t.items.copy()
    wrong["len"][1] += 1                                      # an item that runs past its tensor: refused, nothing is read
    m.t.items = wrong
    with pytest.raises(Exception, match="do not cover"):
        m.step(np.zeros(m.t.n, np.float32))


# -- the item table ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["synthetic", "M", "XL"])
def test_item_table_equals_the_restatement(which):
    _lib()
    off = step_ref.synthetic_seg_off() if which == "synthetic" else step_ref.model_seg_off(which)[0]
    if which == "M":
        assert len(off) - 1 == 316 and off[-1] == 3794322 and sum(int(o) % 4 == 2 for o in off[:-1]) > 0
    items, seg_item = stepops.build_items(off)
    want, want_seg = step_ref.item_table(off)
    assert [(int(i["start"]), int(i["seg"]), int(i["len"])) for i in items] == want
    assert seg_item.tolist() == want_seg


# -- integer inputs: every sum is exact in any order ------------------------------------------------------------------------
def _integer_cases():
    syn = step_ref.synthetic_seg_off()
    eights = np.where(np.random.default_rng(7).integers(0, 2, 16384) == 1, 8.0, -8.0).astype(np.float32)
    return [("synthetic", syn, _integers(16384, 11)), ("eights", syn, eights),
            ("M", step_ref.model_seg_off("M")[0], _integers(3794322, 12))]


def test_integer_inputs_are_exact_in_fp64_in_any_order():
    for name, off, g in _integer_cases():
        n = g.size
        assert n <= 2 ** 22 and np.all(g == np.rint(g)) and np.abs(g).max() <= 1024
        sq = g.astype(np.int64) ** 2                     # int64: exact
        # every partial sum of any order is an integer below n * 1024^2 <= 2^42 < 2^53: exact in fp64
        assert int(sq.sum()) <= n * 1024 ** 2 <= 2 ** 42
        assert math.fsum(sq.astype(np.float64).tolist()) == float(int(sq.sum()))
    assert int((_integer_cases()[1][2].astype(np.int64) ** 2).sum()) == 1024 ** 2


@pytest.mark.parametrize("case", [0, 1, 2], ids=["synthetic", "eights", "M"])
def test_twin_equals_the_restatement_on_integer_inputs(case):
    name, off, g = _integer_cases()[case]
    m = HostMonitor(off)
    head, sumsq, hsh, nf, _ = m.step(g)
    S = len(off) - 1
    sq = g.astype(np.int64) ** 2                         # int64: exact
    want = np.add.reduceat(sq, off[:-1]).astype(np.float64)
    assert want.shape == (S,) and np.array_equal(sumsq, want)
    assert head["total"] == float(int(sq.sum()))
    rs, rh, rn = step_ref.stats(g, off)
    assert np.array_equal(rs, want) and np.array_equal(hsh, rh) and np.array_equal(nf, rn)
    assert head["nonfinite"] == 0 and head["first_bad"] == -1 and head["coef"] == 1.0
    assert head["norm"] == np.sqrt(np.float64(head["total"]))
    # the scalar path (g not 16-byte aligned) gives the same record
    m2 = HostMonitor(off, misalign=1)
    head2, sumsq2, hsh2, nf2, _ = m2.step(g)
    assert head2 == head and np.array_equal(sumsq2, sumsq) and np.array_equal(hsh2, hsh) and np.array_equal(nf2, nf)


@pytest.mark.parametrize("max_norm,inv_world", [(512.0, 1.0), (2048.0, 1.0), (512.0, 0.5), (0.0, 0.5)])
def test_coefficient_on_a_perfect_square_is_the_restatements_bit_for_bit(max_norm, inv_world):
    _, off, g = _integer_cases()[1]
    head, _, _, _, out = HostMonitor(off).step(g, max_norm, inv_world)
    assert head["total"] == 1024.0 ** 2 and head["norm"] == 1024.0 * inv_world
    norm, coef = step_ref.coef_rule(head["total"], inv_world, max_norm)
    assert head["norm"] == norm and np.float32(head["coef"]).tobytes() == coef.tobytes()
    if max_norm == 2048.0 or max_norm == 0.0:
        assert head["coef"] == 1.0 and out.tobytes() == g.tobytes()
    elif inv_world == 0.5:
        # 512 / (512 + 1e-6) = 1 - 2e-9 in fp64, which rounds to 1 in fp32: clipping is on and leaves the bits alone
        assert head["coef"] == 1.0 and out.tobytes() == g.tobytes()
    else:
        assert head["coef"] == np.float32(512.0 / (1024.0 + 1e-6)) == np.float32(0.5)
        assert np.array_equal(out, g * np.float32(head["coef"]))


# -- seeded normal inputs -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which,scale,max_norm,inv_world", [("synthetic", 1.0, 10.0, 1.0), ("synthetic", 1e-3, 1.0, 1.0),
                                                            ("M", 0.02, 2.0, 0.125)])
def test_twin_on_normal_inputs(which, scale, max_norm, inv_world):
    off = step_ref.synthetic_seg_off() if which == "synthetic" else step_ref.model_seg_off(which)[0]
    g = _normals(int(off[-1]), 21, scale)
    head, sumsq, hsh, nf, out = HostMonitor(off).step(g, max_norm, inv_world)
    rs, rh, rn = step_ref.stats(g, off)
    k = np.diff(off).astype(np.float64)
    # k non-negative terms added in any order: the relative error is at most (k - 1) 2^-53
    assert np.all(np.abs(sumsq - rs) <= (k - 1) * U * rs)
    assert np.array_equal(hsh, rh) and np.array_equal(nf, rn) and head["nonfinite"] == 0
    # the total is the per-tensor sums added in tensor order: the same rule over all n terms
    exact_total = math.fsum(rs.tolist())
    assert abs(head["total"] - exact_total) <= (g.size - 1) * U * exact_total
    norm, coef = step_ref.coef_rule(exact_total, inv_world, max_norm)
    assert abs(head["norm"] - norm) <= g.size * U * norm
    assert abs(float(head["coef"]) - float(coef)) <= float(np.spacing(coef))
    assert np.array_equal(out, g * np.float32(head["coef"]))
    if scale == 1e-3:
        assert head["coef"] == 1.0          # the norm is below max_norm: the gradient is left as it is
    else:
        assert head["coef"] < 1.0


# -- the hash -------------------------------------------------------------------------------------------------------------
def test_hash_sees_one_bit_a_swap_and_the_sign_of_zero():
    off = step_ref.synthetic_seg_off()
    g = _normals(16384, 31)
    base = HostMonitor(off).step(g)[2]
    rng = np.random.default_rng(32)
    for s in (0, 3, 7, 9, 10, 11):                      # one flipped bit: that tensor's hash alone
        g2 = g.copy()
        at = int(off[s] + rng.integers(0, off[s + 1] - off[s]))
        g2.view(np.uint32)[at] ^= np.uint32(1 << int(rng.integers(0, 32)))
        h2 = HostMonitor(off).step(g2)[2]
        assert (h2 != base).nonzero()[0].tolist() == [s]
    g2 = g.copy()                                        # two unequal elements of one tensor swapped
    a, b = int(off[10]) + 5, int(off[10]) + 3000
    assert g2[a] != g2[b]
    g2[a], g2[b] = g[b], g[a]
    h2 = HostMonitor(off).step(g2)[2]
    assert (h2 != base).nonzero()[0].tolist() == [10]
    z = np.zeros(16384, np.float32)                      # +0.0 and -0.0
    hp = HostMonitor(off).step(z)
    z[int(off[4]) + 2] = -0.0
    hn = HostMonitor(off).step(z)
    assert (hn[2] != hp[2]).nonzero()[0].tolist() == [4] and np.array_equal(hn[1], hp[1])


# -- non-finite values and the sticky pair ------------------------------------------------------------------------------
def test_nonfinite_counts_first_bad_and_the_sticky_pair():
    off = step_ref.synthetic_seg_off()
    m = HostMonitor(off, R=8)
    clean = _normals(16384, 41)
    assert m.step(clean)[0]["first_bad"] == -1                                   # step 0
    assert m.state[_steplib.S_BAD_STEP] == -1 and m.state[_steplib.S_BAD_SEG] == -1
    bad = clean.copy()
    bad[int(off[9]) + 7] = np.nan
    bad[int(off[9]) + 2047] = -np.inf
    bad[int(off[5])] = np.inf
    bad[int(off[11]) - 1] = np.nan
    head, sumsq, _, nf, _ = m.step(bad, max_norm=1.0)                            # step 1
    want = np.zeros(len(off) - 1, np.int32)
    want[[5, 9, 10]] = [1, 2, 1]
    assert np.array_equal(nf, want) and head["nonfinite"] == 4 and head["first_bad"] == 5
    assert np.isnan(sumsq[9]) and np.isinf(sumsq[5]) and np.isnan(head["total"]) and np.isnan(head["norm"])
    assert np.isnan(head["coef"])                                                # as the arithmetic gives it
    assert (m.state[_steplib.S_BAD_STEP], m.state[_steplib.S_BAD_SEG]) == (1, 5)
    assert m.step(clean)[0]["nonfinite"] == 0                                    # step 2: clean, the pair stays
    assert (m.state[_steplib.S_BAD_STEP], m.state[_steplib.S_BAD_SEG]) == (1, 5)
    worse = clean.copy()
    worse[0] = np.inf
    head = m.step(worse, max_norm=1.0)[0]                                        # step 3: bad again, earlier tensor
    assert head["first_bad"] == 0 and head["norm"] == np.inf and head["coef"] == 0.0
    assert (m.state[_steplib.S_BAD_STEP], m.state[_steplib.S_BAD_SEG]) == (1, 5)
    assert m.state[_steplib.S_STEP] == 4


# -- the ring -----------------------------------------------------------------------------------------------------------------
def test_ring_holds_the_last_R_steps_in_order():
    off = step_ref.seg_off_of([5, 70, 2049])
    R = 4
    m = HostMonitor(off, R=R)
    totals = []
    for i in range(R + 3):
        g = _integers(int(off[-1]), 50 + i, 16)
        totals.append(float(np.sum(g.astype(np.float64) ** 2)))
        m.step(g)
    assert m.state[_steplib.S_STEP] == R + 3
    steps, slots = stepops.ring_steps(m.state, R)
    assert steps == [3, 4, 5, 6] and slots == [3, 0, 1, 2]
    rb = m.t.record_bytes
    for step, slot in zip(steps, slots):
        head = stepops.parse_record(m.ring[slot * rb:(slot + 1) * rb], m.t.S)[0]
        assert head["step"] == step and head["total"] == totals[step]
    assert m.state[_steplib.S_NORM:_steplib.S_NORM + 1].view(np.float64)[0] == np.sqrt(totals[-1])


# -- the same lists under the sanitisers ----------------------------------------------------------------------------------
def _check_file_case(f, off, R, steps, misalign):
    """One case of tests/step_check.cpp's file, with what the in-process twin gave as the expectation."""
    m = HostMonitor(off, R=R, misalign=misalign)
    f.write(struct.pack("<IIII", len(off) - 1, R, len(steps), misalign))
    f.write(np.asarray(off, "<i8").tobytes())
    for g, max_norm, inv_world in steps:
        out = m.step(g, max_norm, inv_world)[4]
        f.write(struct.pack("<dd", max_norm, inv_world))
        f.write(g.astype("<f4").tobytes())
        f.write(out.astype("<f4").tobytes())
    f.write(m.state.astype("<i8").tobytes())
    f.write(m.ring.tobytes())


def test_the_same_lists_in_a_sanitised_stand_alone_program(tmp_path):
    """step_host.cpp and step_core.h compiled with -fsanitize=address,undefined into a program of their own, run as a child
    process on the lists of this file (heap blocks of exactly the sizes the library is told); nothing sanitised is loaded
    into this interpreter."""
    step_program.compiler()
    syn = step_ref.synthetic_seg_off()
    clean, bad = _normals(16384, 61), _normals(16384, 62)
    bad[int(syn[9]) + 7] = np.nan
    bad[int(syn[2])] = -np.inf
    cases = [(syn, 4, [(_integers(16384, 63), 0.0, 1.0), (_integer_cases()[1][2], 512.0, 0.5), (clean, 10.0, 1.0)], 0),
             (syn, 2, [(clean, 10.0, 1.0), (bad, 1.0, 1.0), (clean, 1e30, 1.0), (bad, 0.0, 1.0), (clean, 3.0, 0.25)], 0),
             (syn, 3, [(clean, 10.0, 1.0), (_integers(16384, 64), 100.0, 1.0)], 1),
             (syn, 3, [(clean, 2.0, 1.0)], 3),
             (step_ref.seg_off_of([1]), 1, [(np.array([3.0], np.float32), 1.0, 1.0)] * 2, 0),
             (step_ref.seg_off_of([5, 70, 2049]), 4, [(_integers(2124, 70 + i, 16), 0.0, 1.0) for i in range(7)], 2)]
    path = str(tmp_path / "step_cases.bin")
    with open(path, "wb") as f:
        f.write(struct.pack("<I", len(cases)))
        for off, R, steps, mis in cases:
            _check_file_case(f, off, R, steps, mis)
    last, out = step_program.run(tmp_path, "step_check", path)
    assert last[0] == "cases" and int(last[1]) == len(cases) and int(last[-1]) == 0, out[-500:]


def test_no_kernel_of_the_library_uses_scratch(tmp_path):
    """The four .hip files compiled for gfx950 with the Makefile's flags and the compiler's resource-usage remarks: every
    kernel reports 0 bytes of scratch per lane (an array of 16-byte groups that the compiler leaves in private memory makes
    a walk move its data through scratch, and nothing else would show it), and the kernels that tools and documents cite
    are among them.  The compiler needs no GPU."""
    src = os.path.join(ROOT, "x3d-multigrid_amd", "csrc_step")
    make = open(os.path.join(src, "Makefile")).read()
    hipcc = os.environ.get("HIPCC") or re.search(r"^HIPCC \?= (\S+)", make, re.M).group(1)
    if not (shutil.which(hipcc) or shutil.which("hipcc")):
        pytest.skip("no hipcc")
    hipcc = shutil.which(hipcc) or shutil.which("hipcc")
    arch = re.search(r"^ARCH\s+\?= (\S+)", make, re.M).group(1)
    flags = re.search(r"^CXXFLAGS = (.*)$", make, re.M).group(1).replace("$(ARCH)", arch).split()
    assert arch == "gfx950" and "-ffp-contract=off" in flags
    files = ("step", "ema", "group", "pbn")
    jobs = [subprocess.Popen([hipcc] + flags + ["-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(src, f + ".hip"),
                                                "-o", str(tmp_path / (f + ".o"))], stderr=subprocess.PIPE, text=True)
            for f in files]
    scratch = {}
    for f, job in zip(files, jobs):
        err = job.communicate()[1]
        assert job.returncode == 0, err[-4000:]
        found = re.findall(r"Function Name: (\S+).*?ScratchSize \[bytes/lane\]: (\d+)", err, re.S)
        assert found, "%s.hip: no resource-usage remarks" % f
        scratch.update((name, int(b)) for name, b in found)
    print(scratch)
    assert [k for k, b in scratch.items() if b != 0] == []
    for cited in ("x3dstep_partials_kernel", "x3dstep_finalize_kernel", "x3dstep_scale_kernel", "x3dstep_apply_groups_kernel"):
        assert any(cited in k for k in scratch), cited
