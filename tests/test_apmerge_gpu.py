"""Segment marks and the merge of AP meters on the GPU (csrc_eval/apmerge.hip through x3dhip/evalops.py and apmeter.py):
W segment-tracking meters against ONE plain meter that was fed the same adds in global order -- segment index first,
shard second -- bit for bit on the stored rows and on value(); value() against the fp64 restatement
(tests/apmeter_ref.py) at the bound test_apmeter_gpu.py holds it to; ties that cross shards (the order rule); the flags;
marks captured into a graph; a one-rank RCCL gather."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import apmeter_ref, apmerge_ref
from x3dhip import _evallib

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


def _payload(kind, n, K, weighted, g, dev):
    """The arguments of one add of `n` rows."""
    if kind == "add":
        s = torch.from_numpy(g.choice(np.array([0.1, 0.25, 0.5, 0.75, 0.9], np.float32), size=(n, K))).to(dev)
        y = torch.from_numpy((g.random((n, K)) < 0.3).astype(np.float32)).to(dev)
        w = torch.from_numpy((g.random(n) * 2).astype(np.float32)).to(dev) if weighted else None
        return ("add", (s, y, w))
    if kind == "logits":                                      # n samples of two crops
        z = torch.from_numpy((g.standard_normal((2 * n, K)) * 4).astype(np.float32)).to(dev)
        y = torch.from_numpy((g.random((n, K)) < 0.3).astype(np.float32)).to(dev)
        return ("logits", (z, y))
    TL = max(n, 1)                                            # "frames": sample 0 contributes no row (an all-zero mask)
    pf = torch.from_numpy((g.standard_normal((2, K, 4)) * 4).astype(np.float32)).to(dev)
    lab = torch.from_numpy((g.random((2, K, TL)) < 0.3).astype(np.float32)).to(dev)
    masks = torch.zeros((2, TL), device=dev)
    masks[1, :n] = 1
    return ("frames", (pf, lab, masks))


def _feed(m, payload):
    kind, a = payload
    if kind == "add":
        m.add(a[0], a[1], a[2])
    elif kind == "logits":
        m.add_logits(a[0], a[1], n_crops=2)
    else:
        m.add_frames(a[0], a[1], a[2])


def _build(W, K, lengths, kinds, weighted, seed, reserve=None):
    """W tracking meters fed lengths[r] (one add each) and one plain meter fed the same adds in global order."""
    from apmeter import APMeter
    dev = _dev()
    g = np.random.default_rng(seed)
    shards = [APMeter(track_segments=True) for _ in range(W)]
    for r, rows in (reserve or {}).items():
        shards[r].reserve(rows)
    plain = APMeter()
    i = 0
    for j in range(max(len(l) for l in lengths)):
        for r in range(W):
            if j < len(lengths[r]):
                n = lengths[r][j]
                kind = kinds[i % len(kinds)] if n > 0 else "add" if "add" in kinds else "frames"
                i += 1
                p = _payload(kind, n, K, weighted, g, dev)
                _feed(shards[r], p)
                _feed(plain, p)
    return shards, plain


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _assert_equal_meters(merged, plain, total):
    assert not merged._track
    assert merged._rows() == plain._rows() == total
    assert _same_bits(merged.scores, plain.scores)
    assert torch.equal(merged.targets, plain.targets)
    assert _same_bits(merged.weights, plain.weights)
    got, want = merged.value(), plain.value()
    if total == 0:
        assert got == 0 and want == 0
        return
    assert torch.equal(got, want) and _same_bits(got, want)
    w = plain.weights
    ref = apmeter_ref.average_precision(plain.scores.numpy(), plain.targets.numpy(), w.numpy() if w.numel() else None)
    np.testing.assert_allclose(got.double().numpy(), ref, rtol=0, atol=1e-6)


CASES = {
    # name: (W, K, lengths per shard, add kinds in rotation, weighted, reserve {shard: rows})
    "one_shard": (1, 1, [[0, 1, 63, 64]], ["add", "logits", "frames"], False, None),
    "two_shards_k3": (2, 3, [[64, 65, 257, 0], [1, 63]], ["add", "logits", "frames"], False, None),
    "three_shards_k157_one_empty": (3, 157, [[257, 64], [], [65, 0, 1, 63]], ["frames", "add", "logits"], False, None),
    "eight_shards_weighted_grown": (8, 3, [[257, 257, 257, 257, 65], [1], [0, 64], [63, 65, 1], [64], [], [257, 0, 257],
                                           [1, 1, 1, 1, 1, 1]], ["add"], True, {1: 3000}),
    "eight_shards_k1_frames": (8, 1, [[65, 1], [0], [257], [64, 63], [1], [1, 0, 1], [63], [64]], ["frames", "logits"],
                               False, None),
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_merged_meter_equals_the_plain_meter_fed_in_global_order(name):
    import apmeter
    W, K, lengths, kinds, weighted, reserve = CASES[name]
    shards, plain = _build(W, K, lengths, kinds, weighted, seed=sorted(CASES).index(name), reserve=reserve)
    total = sum(sum(l) for l in lengths)
    if name == "eight_shards_weighted_grown":
        assert shards[0]._cap > 1024 and sum(lengths[0]) > 1024         # the shard grew while it tracked
        assert len({m._cap for m in shards if m._state is not None}) > 1   # shards of different capacities
    merged = apmeter.merge_shards(shards)
    # the marks are the running row counts of each shard
    for m, l in zip(shards, lengths):
        if m._marks is not None:
            mk = m._marks.cpu()
            assert int(mk[0]) == len(l) and mk[1:1 + len(l)].tolist() == np.cumsum(l).astype(int).tolist()
    _assert_equal_meters(merged, plain, total)
    # and the order is the restated one: the shards' own rows permuted by tests/apmerge_ref.py
    if total:
        own = [m.scores.numpy().reshape(-1, K) if m._state is not None else np.zeros((0, K), np.float32) for m in shards]
        want = apmerge_ref.merged_rows(own, lengths)
        assert np.array_equal(merged.scores.numpy().view(np.int32), want.view(np.int32))
    # the shards are left as they were: merging again gives the same meter
    again = apmeter.merge_shards(shards)
    assert _same_bits(again.scores, merged.scores) and torch.equal(again.value(), merged.value())


def test_ties_across_shards_follow_the_interleaved_order():
    """One class, every score equal: the AP is decided by the row order alone.  Interleaved (the rule): targets 1, 1, 0, 0
    -> AP 1; rank-major concatenation would give 1, 0, 1, 0 -> (1 + 2/3) / 2."""
    import apmeter
    from apmeter import APMeter
    dev = _dev()
    half = torch.full((1, 1), 0.5, device=dev)
    one, zero = torch.ones((1, 1), device=dev), torch.zeros((1, 1), device=dev)
    shards = [APMeter(track_segments=True) for _ in range(2)]
    for m in shards:
        m.add(half, one)
        m.add(half, zero)
    merged = apmeter.merge_shards(shards)
    assert merged.targets.view(-1).tolist() == [1, 1, 0, 0]
    got = merged.value()
    interleaved = apmeter_ref.average_precision(np.full((4, 1), 0.5, np.float32), np.array([[1], [1], [0], [0]]))
    rank_major = apmeter_ref.average_precision(np.full((4, 1), 0.5, np.float32), np.array([[1], [0], [1], [0]]))
    assert interleaved[0] == 1.0 and abs(rank_major[0] - (1 + 2 / 3) / 2) < 1e-12
    assert torch.equal(got, torch.ones(1))
    plain = APMeter()
    for y in (one, one, zero, zero):
        plain.add(half, y)
    assert torch.equal(got, plain.value())


def _stacked(shards):
    """The shards' buffers stacked as merge_shards stacks them."""
    import apmeter
    live = [m for m in shards if m._state is not None]
    K, dev = live[0]._K, live[0]._dev
    cap, nmarks = max(m._cap for m in live), max(m._mcap for m in live)
    parts = [apmeter._padded(m, K, False, cap, nmarks, dev) for m in shards]
    return [torch.stack([p[i] for p in parts]) for i in range(4)]


def _raw_destination(dev, K, cap):
    from x3dhip import evalops
    st = evalops.ap_state(dev, cap)
    return st, torch.full((K, cap), 7.5, device=dev), torch.full((K, cap), 9, dtype=torch.uint8, device=dev)


def test_flags_travel_and_failures_write_nothing():
    import apmeter
    from apmeter import APMeter
    from x3dhip import evalops
    dev = _dev()
    # a shard with a non-binary target: the merged value() raises as the plain meter's does
    shards = [APMeter(track_segments=True) for _ in range(2)]
    shards[0].add(torch.rand(5, 3, device=dev), torch.zeros(5, 3, device=dev))
    shards[1].add(torch.rand(5, 3, device=dev), torch.full((5, 3), 2.0, device=dev))
    merged = apmeter.merge_shards(shards)
    assert merged._rows() == 10
    with pytest.raises(ValueError, match="0 / 1"):
        merged.value()
    # a destination too small (raw entry point): OVERFLOW, count 0, buffers untouched
    shards = [APMeter(track_segments=True) for _ in range(2)]
    for m in shards:
        m.add(torch.rand(40, 3, device=dev), torch.zeros(40, 3, device=dev))
    states, marks, scores, targets = _stacked(shards)
    st, ds, dt = _raw_destination(dev, 3, 79)
    evalops.ap_merge(states, marks, scores, targets, None, st, ds, dt)
    host = st.cpu()
    assert int(host[_evallib.S_OVERFLOW]) == 1 and int(host[_evallib.S_COUNT]) == 0 and int(host[_evallib.S_BAD]) == 0
    assert int(host[_evallib.S_CAPACITY]) == 79
    assert bool((ds == 7.5).all()) and bool((dt == 9).all())
    st, ds, dt = _raw_destination(dev, 3, 80)               # exactly enough
    evalops.ap_merge(states, marks, scores, targets, None, st, ds, dt)
    host = st.cpu()
    assert int(host[_evallib.S_COUNT]) == 80 and int(host[_evallib.S_OVERFLOW]) == 0 and int(host[_evallib.S_BAD]) == 0
    assert _same_bits(ds[:, :40], shards[0]._scores[:, :40]) and _same_bits(ds[:, 40:], shards[1]._scores[:, :40])
    # marks made inconsistent by hand: BAD, count 0, nothing written
    for what in ("decreasing", "last_end", "segments", "count"):
        bad_marks, bad_states = marks.clone(), states.clone()
        if what == "decreasing":
            bad_marks[1, 0] = 2
            bad_marks[1, 1:3] = torch.tensor([41, 40], dtype=torch.int32, device=dev)
        elif what == "last_end":
            bad_marks[0, 1] = 39
        elif what == "segments":
            bad_marks[1, 0] = marks.shape[1]                  # s_r = M + 1
        else:
            bad_states[0, _evallib.S_COUNT] = scores.shape[2] + 1     # n_r > C
        st, ds, dt = _raw_destination(dev, 3, 200)
        evalops.ap_merge(bad_states, bad_marks, scores, targets, None, st, ds, dt)
        host = st.cpu()
        assert int(host[_evallib.S_BAD]) == 1 and int(host[_evallib.S_COUNT]) == 0, what
        assert bool((ds == 7.5).all()) and bool((dt == 9).all()), what
    # more marks than max_marks: OVERFLOW on that shard's state, the marks unchanged
    st = evalops.ap_state(dev, 100)
    mk = evalops.ap_marks(dev, 2)
    for _ in range(3):
        evalops.ap_mark(st, mk)
    assert mk.cpu().tolist() == [2, 0, 0] and int(st.cpu()[_evallib.S_OVERFLOW]) == 1
    # host-side refusals
    with pytest.raises(_evallib.X3DHipError):
        evalops.ap_merge(states, marks[:, :1].contiguous()[:1], scores, targets, None, *_raw_destination(dev, 3, 200))
    with pytest.raises(_evallib.X3DHipError):
        evalops.ap_merge(states, marks, scores, targets, None, *_raw_destination(dev, 4, 200))


def _graph_inputs(dev, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    b, n, B, K, T, TL = 3, 2, 2, 7, 4, 9
    z = (torch.randn((b * n, K), generator=g) * 4).to(dev)
    y = (torch.rand((b, K), generator=g) < 0.3).float().to(dev)
    pf = (torch.randn((B, K, T), generator=g) * 4).to(dev)
    lab = (torch.rand((B, K, TL), generator=g) < 0.3).float().to(dev)
    masks = torch.ones(B, TL, device=dev)
    masks[0, 5:] = 0
    return z, y, pf, lab, masks, n, b + 5 + TL


def _capture(m, z, y, pf, lab, masks, n):
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        with torch.cuda.graph(graph, stream=s):
            m.add_logits(z, y, n_crops=n)
            m.add_frames(pf, lab, masks)
    torch.cuda.current_stream().wait_stream(s)
    return graph


def test_marks_captured_into_a_graph_replay_and_merge():
    import apmeter
    from apmeter import APMeter
    dev = _dev()
    z, y, pf, lab, masks, n, per = _graph_inputs(dev, 21)
    R = 4                                                     # one eager round, the capture is not run, three replays
    m = APMeter(track_segments=True)
    m.add_logits(z, y, n_crops=n)
    m.add_frames(pf, lab, masks)
    m.reserve(R * per, segments=2 * R)
    graph = _capture(m, z, y, pf, lab, masks, n)
    for _ in range(3):
        graph.replay()
    torch.cuda.synchronize()
    other = APMeter(track_segments=True)                      # an eager shard next to it
    other.add_logits(z, y, n_crops=n)
    mk = m._marks.cpu()
    assert int(mk[0]) == 2 * R and mk[1:1 + 2 * R].tolist() == [3 + (per) * (i // 2) + (per - 3) * (i % 2) for i in range(2 * R)]
    plain = APMeter()
    plain.add_logits(z, y, n_crops=n)                         # (0, shard 0), (0, shard 1), then shard 0 alone
    plain.add_logits(z, y, n_crops=n)
    plain.add_frames(pf, lab, masks)
    for _ in range(R - 1):
        plain.add_logits(z, y, n_crops=n)
        plain.add_frames(pf, lab, masks)
    _assert_equal_meters(apmeter.merge_shards([m, other]), plain, R * per + 3)
    # growth inside a capture is refused for the marks as it is for the rows
    tight = APMeter(track_segments=True)
    tight.add_logits(z, y, n_crops=n)
    tight._mbound = tight._mcap                               # as if the marks were full
    with pytest.raises(RuntimeError, match="segments"):
        _capture(tight, z, y, pf, lab, masks, n)
    torch.cuda.synchronize()


def test_graph_captured_before_the_marks_grew_is_reported():
    from apmeter import APMeter
    dev = _dev()
    z, y, pf, lab, masks, n, per = _graph_inputs(dev, 22)
    m = APMeter(track_segments=True)
    m.add_logits(z, y, n_crops=n)
    m.add_frames(pf, lab, masks)
    graph = _capture(m, z, y, pf, lab, masks, n)
    graph.replay()
    old_marks, old_cap = m._marks, m._mcap
    m.reserve(0, segments=3 * old_cap)                        # the marks grow after the capture: a new state and marks
    torch.cuda.synchronize()
    assert m._mcap >= 3 * old_cap and m._marks is not old_marks and m._retired
    old_state = m._retired[-1][0]
    assert int(old_state[_evallib.S_CAPACITY].item()) == 0
    count, segs, live = m._count(), m._segments(), m._marks.clone()
    assert count == 2 * per and segs == 4
    graph.replay()
    torch.cuda.synchronize()
    assert m._count() == count and torch.equal(m._marks, live)      # nothing reached the live meter or its marks
    assert int(old_state[_evallib.S_OVERFLOW].item()) == 1
    with pytest.raises(RuntimeError, match="capture again"):
        m.value()
    m.reset()
    m.add_logits(z, y, n_crops=n)
    assert m._segments() == 1 and torch.is_tensor(m.value())


def test_gather_over_a_one_rank_rccl_group_equals_the_meter(tmp_path):
    """In a child process, so that no default process group leaks into the session."""
    _dev()
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT="29641", HSA_ENABLE_IPC_MODE_LEGACY="0")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "charades_ddp_child.py"), "gather1"], env=env,
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-3000:]
    assert "gather1 ok" in out.stdout
