"""Merging AP meters, checks that need no GPU: the merged row order (tests/apmerge_ref.py) is the order of one process for
the two ways the shards are filled (a step's chunks; whole batches r, r + W, ...), the batch cutting / chunking / draw
slicing of charades_train.run consumes a seeded random.Random as the single-process loop does, the loss sum in global
batch order is the loop's sum bit for bit, the new C ABI entries, and merge_shards' errors before any launch."""
import random

import numpy as np
import pytest
import torch

from tests import apmerge_ref
from x3dhip import _evallib


def _rows(ids):
    return np.asarray(ids, np.int64).reshape(-1, 1)


@pytest.mark.parametrize("W,sizes", [(2, [4, 4, 4]), (3, [6, 6, 3]), (8, [16, 8]), (1, [5, 2])])
def test_chunks_of_a_step_merge_to_the_global_batches(W, sizes):
    import charades_train
    ids, nxt = [], 0
    for s in sizes:
        ids.append(list(range(nxt, nxt + s)))
        nxt += s
    shards = [[] for _ in range(W)]
    segs = [[] for _ in range(W)]
    for batch in ids:                                         # one add per step on every rank: its chunk of the batch
        for r in range(W):
            chunk = charades_train._rank_chunk(batch, r, W)
            shards[r] += chunk
            segs[r].append(len(chunk))
    got = apmerge_ref.merged_rows([_rows(s) for s in shards], segs)[:, 0]
    assert list(got) == [i for batch in ids for i in batch]


@pytest.mark.parametrize("W,sizes", [(2, [3, 1, 4, 1, 5]), (3, [2, 7, 1, 8, 2, 8, 1]), (8, [3, 1, 2]), (2, [0, 2, 0, 3, 1])])
def test_whole_batches_round_robin_merge_to_the_global_order(W, sizes):
    ids, nxt = [], 0
    for s in sizes:
        ids.append(list(range(nxt, nxt + s)))
        nxt += s
    shards = [[i for b in ids[r::W] for i in b] for r in range(W)]
    segs = [[len(b) for b in ids[r::W]] for r in range(W)]   # uneven: the first ranks hold one batch more
    assert len({len(s) for s in segs}) > 1 or len(sizes) % W == 0
    got = apmerge_ref.merged_rows([_rows(s) for s in shards], segs)[:, 0]
    assert list(got) == [i for b in ids for i in b]
    # rank-major concatenation is another order as soon as a rank holds two batches
    if max(len(s) for s in segs) > 1 and W > 1:
        assert [i for s in shards for i in s] != list(got)
    idx = apmerge_ref.gather_index(segs, capacity=100)
    assert [int(i) % 100 for i in idx] == [int(x) for x in apmerge_ref.merged_order(segs)[:, 1]]


def test_merged_order_of_no_rows():
    assert apmerge_ref.merged_order([[], []]).shape == (0, 2)
    assert apmerge_ref.merged_order([[0], [0, 0]]).shape == (0, 2)


def _single_process_epochs(n, batch_size, seed, epochs):
    """The loop of charades_train.run for one process: shuffle, batches, draws in batch order."""
    import charades_train
    rng = random.Random(seed)
    draw = lambda i: (i, rng.random(), rng.randint(0, 1 << 30))       # noqa: E731  (a sample's draws consume the shared rng)
    out = []
    for _ in range(epochs):
        order = list(range(n))
        rng.shuffle(order)
        for idx in charades_train._batches(n, batch_size, order):
            out.append((idx, [draw(i) for i in idx]))
    return out, rng.getstate()


@pytest.mark.parametrize("world", [2, 4])
def test_ranks_consume_the_shared_rng_as_one_process_does(world):
    import charades_train
    n, bs, seed, epochs = 24, 8, 5, 2                          # no tail: every global batch is a multiple of world
    single, state = _single_process_epochs(n, bs, seed, epochs)
    per_rank = []
    for rank in range(world):
        rng = random.Random(seed)
        draw = lambda i: (i, rng.random(), rng.randint(0, 1 << 30))   # noqa: E731
        mine = []
        for _ in range(epochs):
            order = list(range(n))
            rng.shuffle(order)
            for idx in charades_train._global_batches(n, bs, order, world):
                mine.append(charades_train._rank_share(draw, idx, rank, world))
        assert rng.getstate() == state                         # the rng went exactly where the single process's went
        per_rank.append(mine)
    for step, (idx, params) in enumerate(single):
        assert sum((per_rank[r][step][0] for r in range(world)), []) == idx          # the chunks tile the global batch
        assert sum((per_rank[r][step][1] for r in range(world)), []) == params       # with the single process's draws


def test_a_tail_is_cut_to_a_multiple_of_world_and_world_one_is_untouched():
    import charades_train
    order = list(range(11))
    assert charades_train._global_batches(11, 4, order, 1) == charades_train._batches(11, 4, order)
    assert charades_train._global_batches(11, 4, order, 2) == [[0, 1, 2, 3], [4, 5, 6, 7], [8, 9]]
    assert charades_train._global_batches(9, 4, list(range(9)), 2) == [[0, 1, 2, 3], [4, 5, 6, 7]]   # 1 < world: no batch
    for world in (2, 3, 4):
        kept = sum(len(b) for b in charades_train._global_batches(11, 12, order, world))
        assert 11 - kept <= world - 1
    assert charades_train._rank_chunk([8, 9, 10, 11], 1, 2) == [10, 11]
    # the ranks that share a cut batch draw the same parameters for it, in the batch's order
    seen = []
    for rank in range(2):
        rng = random.Random(3)
        seen.append(charades_train._rank_share(lambda i: rng.random(), [8, 9], rank, 2))
    rng = random.Random(3)
    assert [seen[0][1][0], seen[1][1][0]] == [rng.random(), rng.random()]


@pytest.mark.parametrize("W,n,width", [(2, 5, 1), (2, 5, 2), (3, 7, 2), (8, 3, 1)])
def test_loss_sum_in_global_order_is_the_loops_sum_bit_for_bit(W, n, width):
    import charades_eval
    g = torch.Generator().manual_seed(n * 10 + W)
    losses = [(torch.rand(width, generator=g) * 3).float() for _ in range(n)]
    sums = None
    for l in losses:                                          # charades_eval's single-process accumulation
        sums = l.clone() if sums is None else sums + l
    per_rank = [torch.stack(losses[r::W]) if losses[r::W] else torch.zeros((0, width)) for r in range(W)]
    got, count = charades_eval.sum_in_global_order(per_rank)
    assert count == n and got.dtype == torch.float32
    assert torch.equal(got.view(torch.int32), sums.view(torch.int32))


def test_merge_abi_entries():
    assert _evallib.ABI_VERSION == 3
    for name in ("x3deval_ap_mark", "x3deval_ap_merge", "x3deval_ap_merge_workspace_bytes"):
        assert name in _evallib.SIGNATURES
    h = _evallib.lib()
    assert h.x3deval_abi_version() == 3
    assert h.x3deval_ap_merge_workspace_bytes(8, 4096) == 4 * (16 + 8 * 4096)
    assert h.x3deval_ap_merge_workspace_bytes(64, 1 << 20) == 4 * (16 + 64 * (1 << 20))
    assert h.x3deval_ap_merge_workspace_bytes(65, 10) == 0 and h.x3deval_ap_merge_workspace_bytes(2, (1 << 20) + 1) == 0
    assert h.x3deval_ap_merge_workspace_bytes(0, 10) == 0
    # beyond the limits the entry points refuse on the host, before any launch (null pointers would fail first otherwise)
    assert h.x3deval_ap_mark(None, None, 4, None) == -1
    assert h.x3deval_ap_merge(*([None] * 5), 65, 4, 3, 8, *([None] * 4), 8, None, 0, None) == -1


def _stub(K, weighted, track=True):
    from apmeter import APMeter
    m = APMeter(track_segments=track)
    if K is not None:
        m._state, m._K, m._weighted, m._dev, m._cap = torch.zeros(8, dtype=torch.int32), K, weighted, torch.device("cpu"), 1024
    return m


def test_merge_shards_errors_come_before_any_launch(monkeypatch):
    import apmeter
    from x3dhip import evalops
    launched = []
    for name in ("ap_merge", "ap_state", "ap_marks", "ap_mark"):
        monkeypatch.setattr(evalops, name, lambda *a, _n=name, **k: launched.append(_n))
    with pytest.raises(ValueError, match="classes"):
        apmeter.merge_shards([_stub(3, False), _stub(4, False)])
    with pytest.raises(ValueError, match="weights"):
        apmeter.merge_shards([_stub(3, False), _stub(None, None), _stub(3, True)])
    with pytest.raises(ValueError, match="track_segments"):
        apmeter.merge_shards([_stub(3, False), _stub(3, False, track=False)])
    with pytest.raises(ValueError):
        apmeter.merge_shards([])
    with pytest.raises(ValueError, match="up to 64"):
        apmeter.merge_shards([_stub(None, None)] * 65)
    with pytest.raises(ValueError, match="track_segments"):
        apmeter.APMeter().reserve(10, segments=5)
    assert launched == []
    empty = apmeter.merge_shards([_stub(None, None), _stub(None, None)])       # shards without rows: an empty meter
    assert empty.value() == 0 and not empty._track and launched == []
