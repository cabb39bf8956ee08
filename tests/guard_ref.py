"""A numpy / pure-Python restatement of the guarded update of include/x3dstep.h (x3dstep_apply, x3dstep_keep), independent of
the library: the per-element rule with every fused multiply-add exact and rounded to fp32 once, the skip decision and its
three counters, and the keep rule."""
from fractions import Fraction

import numpy as np

F32 = np.float32


def round_f32(fr):
    """A non-zero Fraction rounded once to fp32, to nearest, ties to even (no overflow expected: asserted)."""
    assert fr != 0
    sign, a = (-1 if fr < 0 else 1), abs(fr)
    e = a.numerator.bit_length() - a.denominator.bit_length() - 24        # a / 2^e lies in [2^22, 2^25)
    while a >= Fraction(2) ** (e + 24):
        e += 1
    while a < Fraction(2) ** (e + 23):
        e -= 1
    e = max(e, -149)                                                      # subnormals: a fixed step of 2^-149
    q = a / Fraction(2) ** e
    n = q.numerator // q.denominator
    rem = q - n
    if rem > Fraction(1, 2) or (rem == Fraction(1, 2) and n % 2 == 1):
        n += 1
    out = sign * float(n) * 2.0 ** e                                      # n < 2^25 and 2^e: an exact fp64 product
    assert abs(out) < 3.4028235677973366e38
    return F32(out)


def fma_exact(a, b, c):
    """fmaf(a, b, c) of three finite fp32 scalars: a * b + c as a Fraction, rounded once.  An exact zero takes the sign
    IEEE 754 gives it: that of the two terms when they agree, +0 otherwise."""
    a, b, c = F32(a), F32(b), F32(c)
    fr = Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c))
    if fr != 0:
        return round_f32(fr)
    prod_neg = bool(np.signbit(a)) != bool(np.signbit(b))
    if Fraction(float(a)) * Fraction(float(b)) == 0 and float(c) == 0.0 and prod_neg and np.signbit(c):
        return F32(-0.0)
    return F32(0.0)


def fma_f32(a, b, c):
    """fmaf elementwise on fp32 arrays.  The product of two fp32 values is exact in fp64; s = fl64(p + c) and its exact
    error e come from TwoSum.  Rounding s to fp32 is rounding p + c to fp32 once unless s is a tie of the fp32 grid (the 29
    bits below fp32's last are 1 0..0) with e != 0, or the result is near fp32's subnormals: |e| <= ulp64(s) / 2, and
    every other s is at least one ulp64 away from the nearest fp32 tie.  Those elements, and exact zeros (whose sign needs
    the rule), go through fma_exact."""
    a, b, c = (np.asarray(v, dtype=F32) for v in (a, b, c))
    a, b, c = np.broadcast_arrays(a, b, c)
    assert np.all(np.isfinite(a)) and np.all(np.isfinite(b)) and np.all(np.isfinite(c))
    p = a.astype(np.float64) * b.astype(np.float64)
    cd = c.astype(np.float64)
    s = p + cd
    bb = s - p
    e = (p - (s - bb)) + (cd - bb)
    out = s.astype(F32)
    low = s.view(np.uint64) & np.uint64((1 << 29) - 1)
    slow = ((e != 0) & (low == np.uint64(1 << 28))) | (np.abs(s) < 2.0 ** -120)
    flat_out = out.reshape(-1).copy()
    for i in np.flatnonzero(slow.reshape(-1)):
        flat_out[i] = fma_exact(a.reshape(-1)[i], b.reshape(-1)[i], c.reshape(-1)[i])
    return flat_out.reshape(out.shape)


def apply_rule(w, g, m, coef, lr, mu, wd, gs, first):
    """(w', m') of the applied update: gi = g (coef == 1) or g * coef; t = gi * gs; gi' = fmaf(wd, w, t);
    m' = gi' (first) or fmaf(mu, m, gi'); w' = w - lr * m'.  Every plain operation is numpy's fp32 one (rounded once)."""
    w, g, m = (np.asarray(v, dtype=F32) for v in (w, g, m))
    coef, lr, mu, wd, gs = F32(coef), F32(lr), F32(mu), F32(wd), F32(gs)
    gi = g if coef == F32(1.0) else g * coef
    t = gi * gs
    gg = fma_f32(wd, w, t)
    mi = gg if first else fma_f32(mu, m, gg)
    step = lr * mi
    return (w - step).astype(F32), mi.astype(F32)


def skips(g):
    """The decision: an update is skipped when its gradient holds a NaN, a +Inf or a -Inf."""
    return not bool(np.all(np.isfinite(np.asarray(g, dtype=F32))))


class Counters:
    """The three state words: skip (of the latest apply), skipped (the total), run (skipped in a row)."""

    def __init__(self):
        self.skip = self.skipped = self.run = 0

    def step(self, skip):
        self.skip = 1 if skip else 0
        if skip:
            self.skipped += 1
            self.run += 1
        else:
            self.run = 0
        return self.skip, self.skipped, self.run


def keep_rule(live, snap, offsets, mode, skip_word):
    """The keep rule on a list of live arrays and a snapshot: mode 0 copies every live[b] to snap[offsets[b]:][:len];
    mode 1 copies back when skip_word == 1, else nothing.  Returns (new live list, new snap) as copies."""
    live = [np.array(b, dtype=F32, copy=True) for b in live]
    snap = np.array(snap, dtype=F32, copy=True)
    for b, off in zip(live, offsets):
        if mode == 0:
            snap[off:off + b.size] = b
        elif skip_word == 1:
            b[:] = snap[off:off + b.size]
    return live, snap
