"""A numpy / pure-Python restatement of the weight average of include/x3dstep.h (x3dstep_ema, x3dstep_ema_keep), independent
of the library: the count, skip and decay rules in Python integers and fp64, the element rule with the product and the
fused multiply-add each rounded to fp32 once (the exact-arithmetic helpers of tests/guard_ref.py)."""
import numpy as np

from tests.guard_ref import fma_f32

F32 = np.float32
S_STEP, S_SKIP, S_SKIPPED = 0, 5, 6


def count_rule(state, count):
    """k: the host's count, plus (with a state) the updates applied so far."""
    count = int(count)
    return count if state is None else count + int(state[S_STEP]) - int(state[S_SKIPPED])


def skips(state):
    return state is not None and int(state[S_SKIP]) == 1


def decay_rule(k, decay, warmup):
    """(d, omd) as fp32 scalars: fp64, rounded once per value.  `decay` is the fp32 value the library is handed."""
    k = int(k)
    assert k >= 1
    d = float(F32(decay))
    if warmup:
        d = min(d, (1 + k) / (10.0 + k))            # an int over a float: one correctly rounded fp64 division
    d = F32(d)
    return d, F32(1.0 - float(d))


def element_rule(e, w, d, omd):
    """e' = fmaf(d, e, omd * w) on finite fp32 arrays."""
    e, w = np.asarray(e, dtype=F32), np.asarray(w, dtype=F32)
    p = (F32(omd) * w).astype(F32)                  # numpy's fp32 product: rounded once
    return fma_f32(F32(d), e, p)


def update(e, w, state, count, decay, warmup):
    """The new average, or None when the rules say that nothing is stored (a skipped update) -- k <= 0 is an error."""
    k = count_rule(state, count)
    if k <= 0:
        raise ValueError("k = %d: nothing to average" % k)
    if skips(state):
        return None
    d, omd = decay_rule(k, decay, warmup)
    return element_rule(e, w, d, omd)

