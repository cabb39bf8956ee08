"""The row order of a merge of AP meters (include/x3deval.h, x3deval_ap_merge), restated in numpy: segment index first,
shard second.  Lists of per-shard segment lengths in, the row permutation out."""
import numpy as np


def merged_order(segments):
    """segments[r] = the lengths of shard r's segments (one per add), in the shard's order.  Returns (shard, row) int64
    [N, 2]: destination row d holds row `row` of shard `shard`.  Order: (segment 0, shard 0), (segment 0, shard 1), ...,
    (segment 1, shard 0), ...; a shard with fewer segments is absent from the later rounds."""
    starts = [np.concatenate([[0], np.cumsum(np.asarray(s, np.int64))]) for s in segments]
    out = []
    for j in range(max([len(s) for s in segments] + [0])):
        for r, s in enumerate(segments):
            if j < len(s):
                rows = np.arange(starts[r][j], starts[r][j + 1], dtype=np.int64)
                out.append(np.stack([np.full_like(rows, r), rows], 1))
    return np.concatenate(out, 0) if out else np.zeros((0, 2), np.int64)


def merged_rows(shards, segments):
    """shards[r]: array [n_r, ...] of shard r's rows; returns them in the merged order."""
    order = merged_order(segments)
    if not len(order):
        return np.zeros((0,) + tuple(np.asarray(shards[0]).shape[1:]), np.asarray(shards[0]).dtype)
    return np.stack([np.asarray(shards[r])[i] for r, i in order])


def gather_index(segments, capacity):
    """The merged order as an index into the stacked, padded buffers [W * capacity] (row i of shard r at r * capacity + i):
    what a host-built torch.index_select along the row axis would use."""
    order = merged_order(segments)
    return order[:, 0] * int(capacity) + order[:, 1]
