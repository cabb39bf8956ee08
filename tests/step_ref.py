"""A numpy / pure-Python restatement of include/x3dstep.h, independent of the library: the item table, the per-tensor
statistics (math.fsum and exact integer sums, numpy uint64 for the hash) and the coefficient rule in numpy fp64."""
import math

import numpy as np

ITEM = 2048
# the tensor lengths every table of the tests must contain: around a group of four, a wave's round of 64 groups... and the item
EDGE_LENGTHS = [1, 2, 3, 24, 63, 64, 65, ITEM - 1, ITEM, ITEM + 1, 2 * ITEM + 1]
# ... and a last tensor that brings the table to 16384 elements (every element +-8 then has norm 1024 exactly)
SYNTHETIC_LENGTHS = EDGE_LENGTHS + [16384 - sum(EDGE_LENGTHS)]


def seg_off_of(lengths):
    return np.concatenate([[0], np.cumsum(np.asarray(lengths, dtype=np.int64))]).astype(np.int64)


def synthetic_seg_off():
    off = seg_off_of(SYNTHETIC_LENGTHS)
    assert off[-1] == 16384 and set(int(o) % 4 for o in off[:-1]) == {0, 1, 2, 3}
    return off


def model_seg_off(version):
    """The flat layout trainer.FlatParams gives a model: named_parameters() order, unpadded offsets."""
    import x3d
    net = x3d.generate_model(version, n_classes=400)
    names = [k for k, _ in net.named_parameters()]
    return seg_off_of([p.numel() for _, p in net.named_parameters()]), names


def item_table(seg_off):
    """[(start, seg, len)], seg_item [S + 1]"""
    items, seg_item = [], []
    for s in range(len(seg_off) - 1):
        a, b = int(seg_off[s]), int(seg_off[s + 1])
        seg_item.append(len(items))
        while a < b:
            k = min(ITEM, b - a)
            items.append((a, s, k))
            a += k
    seg_item.append(len(items))
    return items, seg_item


def splitmix64(z):
    z = np.asarray(z, dtype=np.uint64).copy()
    with np.errstate(over="ignore"):
        z += np.uint64(0x9e3779b97f4a7c15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xbf58476d1ce4e5b9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94d049bb133111eb)
    return z ^ (z >> np.uint64(31))


def tensor_hash(x):
    bits = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    idx = np.arange(bits.size, dtype=np.uint64)
    h = splitmix64((idx << np.uint64(32)) | bits)
    return int(np.add.reduce(h, dtype=np.uint64))          # numpy's uint64 sum wraps: mod 2^64


def tensor_sumsq(x):
    """The correctly rounded sum of the exact squares (a product of two fp32 values is exact in fp64)."""
    d = np.asarray(x, dtype=np.float32).astype(np.float64)
    return math.fsum((d * d).tolist())


def tensor_nonfinite(x):
    return int(np.count_nonzero(~np.isfinite(np.asarray(x, dtype=np.float32))))


def stats(g, seg_off):
    """(sumsq [S] fp64 by fsum, hash [S] uint64, nonfinite [S] int32) of the tensors of g."""
    S = len(seg_off) - 1
    parts = [g[int(seg_off[s]):int(seg_off[s + 1])] for s in range(S)]
    return (np.array([tensor_sumsq(p) for p in parts], np.float64), np.array([tensor_hash(p) for p in parts], np.uint64),
            np.array([tensor_nonfinite(p) for p in parts], np.int32))


def coef_rule(total, inv_world, max_norm):
    """(norm fp64, coef fp32): norm = sqrt(total) * inv_world; coef = fp32(min(1, max_norm / (norm + 1e-6))), 1 when off."""
    with np.errstate(all="ignore"):
        norm = np.sqrt(np.float64(total)) * np.float64(inv_world)
        if not max_norm > 0:
            return norm, np.float32(1.0)
        c = np.minimum(np.float64(1.0), np.float64(max_norm) / (norm + np.float64(1e-6)))
        return norm, np.float32(c)
