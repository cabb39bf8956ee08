"""What tests/test_group_host.py and tests/test_group_gpu.py share: the per-tensor scales, the case grid of the grouped update
and the CPU twin's buffers with guard bands (HostGroup)."""
import itertools

import numpy as np

from tests import guard_cases as gc
from x3dhip import _steplib, stepops

N = 16384
LR_SCALES = (1.0, 0.0, 0.5, 10.0, 0.1)
WD_SCALES = (1.0, 0.0, 2.0)
SHIFTS = [(0, 0, 0), (1, 1, 1), (2, 2, 2), (3, 3, 3), (0, 1, 2)]      # the four congruent alignments, one that is not


def scales(S):
    """Every tensor its own pair: tensor s takes LR_SCALES[s mod 5] and WD_SCALES[s mod 3] (15 distinct pairs in a row), so
    that a 16-byte group across two tensors, or a lane with its neighbour's scales, gives other bytes."""
    hy = np.zeros(S, dtype=_steplib.HYPER_DT)
    hy["lr_scale"] = [LR_SCALES[s % 5] for s in range(S)]
    hy["wd_scale"] = [WD_SCALES[s % 3] for s in range(S)]
    return hy


def ones(S):
    hy = np.zeros(S, dtype=_steplib.HYPER_DT)
    hy["lr_scale"] = hy["wd_scale"] = 1.0
    return hy


# first x nesterov / momentum x grad_scale x weight_decay x (no state | state, coefficient 1 | state, coefficient 0.5)
GRID = [dict(first=f, nesterov=nv, mu=mu, gs=gs, wd=wd, state=st, clipped=c)
        for f, (nv, mu), gs, wd, (st, c) in itertools.product(
            (0, 1), ((0, 0.9), (1, 0.9), (0, 0.0)), (1.0, 0.5), (0.0, 5e-5), ((False, False), (True, False), (True, True)))]


def case_id(a):
    return "first%d-nest%d-mu%g-gs%g-wd%g-%s" % (a["first"], a["nesterov"], a["mu"], a["gs"], a["wd"],
                                                ("clipped" if a["clipped"] else "coef1") if a["state"] else "nostate")


def gradient_for(a, n, seed):
    """(g, max_norm): the perfect-square gradient of tests/guard_cases.py (coefficient 0.5) for a clipped case."""
    return gc.gradient_for(dict(clipped=a["clipped"]), n, seed)


class HostGroup(gc.HostGuard):
    """HostGuard with a hyper table: the twin's w, g, m inside guard bands, the state, the ring and the scales."""

    def __init__(self, seg_off, hyper=None, R=4, shifts=(0, 0, 0)):
        super().__init__(seg_off, R=R, shifts=shifts)
        self.hyper = scales(self.t.S) if hyper is None else hyper

    def apply_groups(self, a, lr=gc.LR, state=True):
        stepops.apply_groups_host(self.w, self.g, self.m, self.t, self.hyper, self.state if state else None,
                                  self.ring if state else None, self.R, lr, a["mu"], a["wd"], a["gs"], a["first"],
                                  a.get("nesterov", 0))

    def run(self, a, g, max_norm=0.0, lr=gc.LR):
        """One case of GRID: load g, measure when the case has a state, apply."""
        self.load(g=g)
        if a["state"]:
            self.measure(max_norm)
        self.apply_groups(a, lr, state=a["state"])


def bad_item_tables(t):
    """[(name, items, hyper, index of the bad item)]: the table of StepTables t with one item (or its tensor's scales)
    spoilt in each way the per-item tests name.  The item chosen is one of several of its tensor where that matters."""
    out = []
    k = t.nitems - 2                      # an inner item of the last tensor
    for name, field, value in (("seg-negative", "seg", -1), ("seg-past-S", "seg", t.S), ("len-zero", "len", 0),
                               ("len-past-item", "len", _steplib.ITEM + 1), ("start-negative", "start", -4),
                               ("start-past-end", "start", t.n - int(t.items["len"][k]) + 1)):
        items = t.items.copy()
        items[field][k] = value
        out.append((name, items, scales(t.S), [k]))
    for name, field, value in (("lr-scale-negative", "lr_scale", -1.0), ("lr-scale-nan", "lr_scale", np.nan),
                               ("wd-scale-inf", "wd_scale", np.inf), ("wd-scale-negative", "wd_scale", -0.5)):
        hy = scales(t.S)
        s = 9                             # ITEM + 1 elements: two items
        hy[field][s] = value
        out.append((name, t.items.copy(), hy, list(range(int(t.seg_item[s]), int(t.seg_item[s + 1])))))
    return out
