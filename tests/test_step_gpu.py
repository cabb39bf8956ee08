"""The three kernels of libx3dstep on the GPU against the library's CPU twin (which tests/test_step_host.py holds against
the numpy restatement): records byte for byte, the scaled gradient, guard bands around the flat buffer and the ring, and
the same three launches captured into a graph."""
import numpy as np
import pytest
import torch

from tests import step_ref
from x3dhip import _steplib, stepops

pytestmark = pytest.mark.gpu

GUARD = 64           # elements (of g) / bytes x 4 (of the ring) on both sides


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


def _seg_off(which):
    if which == "many":
        # 2700 short tensors: more tensors than one round of the finalize step takes (1024) and more items than it keeps
        # in LDS (2560), so the later ones are read from the scratch
        return step_ref.seg_off_of([(i % 7) + 1 for i in range(2700)])
    return step_ref.synthetic_seg_off() if which == "synthetic" else step_ref.model_seg_off(which)[0]


def _gradients(off, seed):
    """(g, max_norm, inv_world) per step: integers, normals that are clipped and that are not, non-finite values planted in
    chosen tensors, clipping off."""
    n, S = int(off[-1]), len(off) - 1
    rng = np.random.default_rng(seed)
    ints = rng.integers(-1024, 1025, n).astype(np.float32)
    small = (rng.standard_normal(n) * 1e-3).astype(np.float32)
    big = rng.standard_normal(n).astype(np.float32)
    bad = big.copy()
    bad[int(off[S // 2]) + 1 if off[S // 2 + 1] - off[S // 2] > 1 else int(off[S // 2])] = np.nan
    bad[int(off[S - 1])] = np.inf
    bad[int(off[S - 2])] = -np.inf
    return [(ints, 0.0, 1.0), (big, 3.0, 1.0), (small, 1e6, 1.0), (bad, 2.0, 1.0), (big, 0.5, 0.125), (ints, 100.0, 0.5)]


class Twin:
    def __init__(self, off, R):
        self.t = stepops.StepTables(off)
        self.R = R
        self.state = stepops.new_state()
        self.ws = stepops.aligned_bytes(self.t.workspace_bytes)
        self.ring = stepops.aligned_bytes(R * self.t.record_bytes)
        self.g = stepops.aligned_bytes(4 * self.t.n).view(np.float32)

    def step(self, g, max_norm, inv_world):
        self.g[:] = g
        stepops.observe_host(self.g, self.t, self.ws, self.state, self.ring, self.R, max_norm, inv_world)
        return self.g.copy()


class Device:
    """The device buffers with guard bands: g inside a larger float buffer (`shift` extra elements in front move it off the
    16-byte grid), the ring inside a larger byte buffer."""

    def __init__(self, off, R, dev, shift=0):
        self.t = stepops.StepTables(off, dev)
        self.R = R
        n, rb = self.t.n, R * self.t.record_bytes
        self.gbig = torch.full((GUARD + shift + n + GUARD,), 7.25, dtype=torch.float32, device=dev)
        self.g = self.gbig[GUARD + shift:GUARD + shift + n]
        assert self.g.data_ptr() % 16 == 4 * (shift % 4)
        self.rbig = torch.full((4 * GUARD + rb + 4 * GUARD,), 0xA5, dtype=torch.uint8, device=dev)
        self.ring = self.rbig[4 * GUARD:4 * GUARD + rb]
        self.ring.zero_()
        self.ws = torch.zeros(self.t.workspace_bytes, dtype=torch.uint8, device=dev)
        self.state = torch.from_numpy(stepops.new_state()).to(dev)
        self.shift = shift

    def load(self, g):
        self.g.copy_(torch.from_numpy(g))

    def step(self, g, max_norm, inv_world):
        self.load(g)
        stepops.observe(self.g, self.t, self.ws, self.state, self.ring, self.R, max_norm, inv_world)
        return self.g.clone()

    def guards_intact(self):
        lo, hi = GUARD + self.shift, GUARD + self.shift + self.t.n
        rb = self.R * self.t.record_bytes
        return (bool((self.gbig[:lo] == 7.25).all()) and bool((self.gbig[hi:] == 7.25).all())
                and bool((self.rbig[:4 * GUARD] == 0xA5).all()) and bool((self.rbig[4 * GUARD + rb:] == 0xA5).all()))


def _same(twin, d, outs_t, outs_d):
    torch.cuda.synchronize()
    assert torch.equal(d.state.cpu(), torch.from_numpy(twin.state))
    assert torch.equal(d.ring.cpu(), torch.from_numpy(np.ascontiguousarray(twin.ring)))       # byte for byte
    for a, b in zip(outs_t, outs_d):
        # bytes, so that a NaN equals itself
        assert torch.equal(b.cpu().view(torch.int32), torch.from_numpy(a).view(torch.int32))
    assert d.guards_intact()


@pytest.mark.parametrize("which,shift", [("synthetic", 0), ("synthetic", 1), ("synthetic", 2), ("synthetic", 3), ("M", 0),
                                         ("many", 0)])
def test_kernels_equal_the_twin(which, shift):
    dev = _dev()
    off = _seg_off(which)
    R = 4                                    # six steps: the ring wraps
    twin, d = Twin(off, R), Device(off, R, dev, shift)
    outs_t, outs_d = [], []
    for g, max_norm, inv_world in _gradients(off, 100 + shift):
        outs_t.append(twin.step(g, max_norm, inv_world))
        outs_d.append(d.step(g, max_norm, inv_world))
    _same(twin, d, outs_t, outs_d)
    st = d.state.cpu().numpy()
    S = len(off) - 1
    assert st[_steplib.S_STEP] == 6 and st[_steplib.S_BAD_STEP] == 3 and st[_steplib.S_BAD_SEG] == S // 2
    # what the records say, against the restatement: the integers of the last step are exact
    g, max_norm, inv_world = _gradients(off, 100 + shift)[-1]
    head, sumsq, hsh, nf = stepops.parse_record(d.ring.cpu().numpy()[(5 % R) * d.t.record_bytes:][:d.t.record_bytes], S)
    rs, rh, rn = step_ref.stats(g, off)
    assert np.array_equal(sumsq, rs) and np.array_equal(hsh, rh) and np.array_equal(nf, rn)
    norm, coef = step_ref.coef_rule(float(rs.sum()), inv_world, max_norm)
    assert head["total"] == rs.sum() and head["norm"] == norm and head["coef"] == coef and head["step"] == 5


@pytest.mark.parametrize("which", ["synthetic", "M", "many"])
def test_captured_launches_give_the_same_records_on_new_contents(which):
    dev = _dev()
    off = _seg_off(which)
    R = 8
    twin, d = Twin(off, R), Device(off, R, dev)
    steps = _gradients(off, 200)
    max_norm, inv_world = 2.0, 0.5           # what a capture fixes; the contents change
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    d.load(steps[0][0])
    with torch.cuda.stream(s):               # one eager step first (step 0), as a capture's warm-up does
        stepops.observe(d.g, d.t, d.ws, d.state, d.ring, R, max_norm, inv_world)
    torch.cuda.current_stream().wait_stream(s)
    outs_t, outs_d = [twin.step(steps[0][0], max_norm, inv_world)], [d.g.clone()]
    graph = torch.cuda.CUDAGraph()
    d.load(steps[1][0])
    with torch.cuda.graph(graph):
        stepops.observe(d.g, d.t, d.ws, d.state, d.ring, R, max_norm, inv_world)
    for g, _, _ in steps[1:]:
        d.load(g)
        graph.replay()
        outs_d.append(d.g.clone())
        outs_t.append(twin.step(g, max_norm, inv_world))
    _same(twin, d, outs_t, outs_d)
    assert int(d.state[_steplib.S_STEP]) == len(steps)


def test_observe_refuses_what_it_cannot_run():
    dev = _dev()
    off = _seg_off("synthetic")
    d = Device(off, 2, dev)
    with pytest.raises(ValueError):
        stepops.observe(d.g[:-1], d.t, d.ws, d.state, d.ring, 2)                 # another length than the tables'
    with pytest.raises(ValueError):
        stepops.observe(d.g, d.t, d.ws, d.state, d.ring, 3)                      # a ring too small for R
    with pytest.raises(ValueError):
        stepops.observe(d.g.cpu(), d.t, d.ws, d.state, d.ring, 2)                # no fallback on the CPU
    torch.cuda.synchronize()
    assert int(d.state[_steplib.S_STEP]) == 0 and d.guards_intact()
