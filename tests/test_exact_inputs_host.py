"""The proof behind tests/test_exact_gpu.py, on the CPU: on the inputs of tests/exact_inputs.py every op, evaluated in
torch fp32 in two different summation orders and in fp64, gives bitwise the same result, and the any-order exactness
condition sum |terms| / u < 2^24 holds for every output kind of every case the GPU tests use.  For the split-term probes
the bf16 split is emulated: the six products the kernels keep reproduce the fp64 result exactly, leaving out any one a
probe kind is there for changes at least 3 of 4 outputs in every 16-row x 32-voxel tile, and the two-term form cannot
reproduce the probes that carry a lo term.  So a mismatch on the GPU is the kernel's fault."""
import pytest
import torch

from tests import exact_inputs as ei
from tests.exact_inputs import DW_ALL, FUSED_ALL, HEAD_EXACT, PW_ALL, STEM_EXACT


def _three_ways(ref, mags, case, what):
    r64 = ref(case, torch.float64, 0)
    ei.assert_exact(mags(case, r64), what)
    for order in (0, 1):
        r32 = ref(case, torch.float32, order)
        assert set(r32) == set(r64)
        for k, v in r32.items():
            assert v.dtype == torch.float32
            assert torch.equal(v.double(), r64[k]), "%s %s: fp32 (order %d) differs from fp64" % (what, k, order)
    r64b = ref(case, torch.float64, 1)
    for k, v in r64b.items():
        assert torch.equal(v, r64[k]), "%s %s: the two evaluation orders disagree in fp64" % (what, k)


def test_unit_of_and_the_exactness_condition():
    assert ei.unit_of(torch.tensor([0.5, 3.0, 0.75])) == 0.25
    assert ei.unit_of(torch.tensor([4.0, -8.0])) == 4.0
    assert ei.unit_of(torch.zeros(3)) == 1.0
    assert ei.unit_of(torch.tensor([ei.PROBE_V], dtype=torch.float64)) == 2.0 ** -20
    ei.assert_exact({"ok": (torch.tensor([2.0 ** 24 - 1]), 1.0)})
    with pytest.raises(AssertionError):
        ei.assert_exact({"too long a sum": (torch.tensor([2.0 ** 22]), 0.25)})
    # the condition is not decoration: 2^24 + 1 is the first integer fp32 cannot hold
    assert float(torch.tensor(2.0 ** 24) + torch.tensor(1.0)) == 2.0 ** 24


def test_sparse_rows_hit_every_column_and_tap():
    for M, K, nnz in [(54, 24, 4), (24, 54, 4), (192, 432, 4), (432, 96, 4), (2, 27, 3), (3, 27, 3), (24, 27, 4), (24, 5, 2)]:
        w = ei.sparse_rows(M, K, nnz, 5)
        assert bool((w != 0).any(0).all()) and set(w.unique().tolist()) <= {0.0, 0.5, -0.5, 1.0, -1.0}
        assert int((w != 0).sum(1).max()) == max(nnz, -(-K // M))


@pytest.mark.parametrize("case", PW_ALL)
def test_pw_integer_cases_are_exact_in_any_order(case):
    c = ei.pw_case(case)
    xin = ei.affine(c.pre, c.x) if c.act else c.x
    assert set(xin.unique().tolist()) <= {0.0, 1.0, -1.0, 2.0, -2.0}              # the effective activations
    _three_ways(ei.pw_ref, ei.pw_mags, c, "pw %s" % (case,))


@pytest.mark.parametrize("case", FUSED_ALL)
def test_pw_fused_integer_cases_are_exact_in_any_order(case):
    _three_ways(ei.fused_ref, ei.fused_mags, ei.fused_case(case), "fused %s" % (case,))


@pytest.mark.parametrize("case", DW_ALL)
def test_dw333_integer_cases_are_exact_in_any_order(case):
    c = ei.dw_case(case)
    assert bool((c.w.view(case[1], 27) != 0).any(0).all())                          # all 27 taps
    _three_ways(ei.dw_ref, ei.dw_mags, c, "dw333 %s" % (case,))


@pytest.mark.parametrize("shape", STEM_EXACT)
def test_stem_integer_cases_are_exact_in_any_order(shape):
    _three_ways(ei.stem_ref, ei.stem_mags, ei.stem_case(shape), "stem %s" % (shape,))


@pytest.mark.parametrize("R", ei.HEAD_R)
def test_head_integer_cases_are_exact_in_any_order(R):
    for (r, K, J, C) in HEAD_EXACT:
        if r == R:
            _three_ways(ei.head_ref, ei.head_mags, ei.head_case(R, K, J, C), "head %s" % ((R, K, J, C),))


# --------------------------------------------------------------------------------------------------------- probes
def test_probe_values_split_into_three_nonzero_terms():
    s = ei.split3(torch.tensor([ei.PROBE_V, -ei.PROBE_V, ei.PROBE_B, 1.0, 0.0], dtype=torch.float64))
    assert s["hi"].tolist() == [1.0, -1.0, 1.0, 1.0, 0.0]
    assert s["mid"].tolist() == [2.0 ** -10, -2.0 ** -10, 2.0 ** -10, 0.0, 0.0]
    assert s["lo"].tolist() == [2.0 ** -20, -2.0 ** -20, 0.0, 0.0, 0.0]
    assert sorted(set(p for k in ei.PROBE_KINDS for p in ei.NEEDS[k])) == sorted(ei.KEPT)      # every kept product is probed


def _probe_proof(A, B, ref, kind, what):
    """A [M, K], B [K, cols] fp64 probe operands, ref = A B [M, cols]."""
    assert torch.equal(A.float().double(), A) and torch.equal(B.float().double(), B)           # fp32 values
    assert torch.equal(A @ B, ref)
    cnt = ei.probe_count(A, B)
    assert float(cnt.max()) <= 8
    ei.assert_exact({"probe": (A.abs() @ B.abs(), 2.0 ** -20)}, what)
    assert float((A.abs() @ B.abs()).max()) < 16
    # the signed count m of an output is +-(its number of non-zero products): never 0 where a product exists
    m = torch.sign(A) @ torch.sign(B)
    assert torch.equal(m.abs(), cnt)
    # fp32 in two orders
    perm = torch.arange(A.shape[1] - 1, -1, -1)
    for got in (A.float() @ B.float(), A.float()[:, perm] @ B.float()[perm]):
        assert torch.equal(got.double(), ref), what
    sa, sb = ei.split3(A), ei.split3(B)
    prod = {(p, q): sa[p] @ sb[q] for p in ("hi", "mid", "lo") for q in ("hi", "mid", "lo")}
    for pq in (("mid", "lo"), ("lo", "mid"), ("lo", "lo")):                                    # dropped by design: zero here
        assert not bool(prod[pq].any()), (what, pq)
    assert torch.equal(sum(prod[pq] for pq in ei.KEPT), ref), what + ": the six kept products do not reproduce the result"
    for pq in ei.KEPT:
        without = sum(prod[o] for o in ei.KEPT if o != pq)
        if pq in ei.NEEDS[kind]:
            assert not torch.equal(without, ref)
            yield pq, without != ref
        else:
            assert not bool(prod[pq].any()), (what, pq)
    if kind in ei.CARRIES_LO:
        two = prod[("hi", "hi")] + prod[("hi", "mid")] + prod[("mid", "hi")]
        yield "two-term", two != ref


def _resolved(changed, N, what):
    """changed [M, N * P] -> every 16 x 32 tile of every sample: at least 3 of 4 outputs change."""
    M = changed.shape[0]
    frac = ei.tiles_resolved(changed.view(M, N, -1).transpose(0, 1))
    assert frac >= 0.75, "%s: a tile where only %.2f of the outputs resolve the term" % (what, frac)


_FWD_SHAPES = sorted(set(s for v in ei.PROBE_FWD.values() for s in v))


@pytest.mark.parametrize("kind", ei.PROBE_KINDS)
@pytest.mark.parametrize("shape", _FWD_SHAPES)
def test_forward_probes_resolve_every_kept_product(shape, kind):
    N, Ci, Co, T, H, W = shape
    w, x, y = ei.probe_fwd(shape, kind)
    A, B = w, x.flatten(2).transpose(0, 1).reshape(Ci, -1)
    ref = y.flatten(2).transpose(0, 1).reshape(Co, -1)
    for pq, changed in _probe_proof(A, B, ref, kind, "fwd %s %s" % (shape, kind)):
        _resolved(changed, N, "fwd %s %s without %s" % (shape, kind, pq))


@pytest.mark.parametrize("kind", ei.PROBE_KINDS)
@pytest.mark.parametrize("shape", sorted(set(ei.PROBE_DGRAD + ei.PROBE_FUSED)))
def test_data_gradient_probes_resolve_every_kept_product(shape, kind):
    N, Ci, Co, T, H, W = shape
    w, dY, dX = ei.probe_dgrad(shape, kind)
    A, B = w.t(), dY.flatten(2).transpose(0, 1).reshape(Co, -1)
    ref = dX.flatten(2).transpose(0, 1).reshape(Ci, -1)
    for pq, changed in _probe_proof(A, B, ref, kind, "dgrad %s %s" % (shape, kind)):
        _resolved(changed, N, "dgrad %s %s without %s" % (shape, kind, pq))


@pytest.mark.parametrize("kind", ei.PROBE_KINDS)
@pytest.mark.parametrize("shape", sorted(set(ei.PROBE_WGRAD + ei.PROBE_FUSED)))
def test_weight_gradient_probes_resolve_every_kept_product(shape, kind):
    N, Ci, Co, T, H, W = shape
    dY, x, dW = ei.probe_wgrad(shape, kind)
    A = dY.flatten(2).transpose(0, 1).reshape(Co, -1)
    B = x.flatten(2).transpose(0, 1).reshape(Ci, -1).t()
    for pq, changed in _probe_proof(A, B, dW, kind, "wgrad %s %s" % (shape, kind)):
        _resolved(changed, 1, "wgrad %s %s without %s" % (shape, kind, pq))
