"""libx3dmix on the GPU: mix_clips and mix_targets against their CPU twins bit for bit on every hand-built case of
tests/mix_cases.py (aligned tensors and views one float into a larger buffer), a batch that takes more than one pass of
the clip kernel's grid, the refusals, and soft_ce against torch in fp64 on the host test's inputs and bounds, reproducible
bit for bit, with the head's draw counter.  Everything under ops.set_guard(True)."""
import numpy as np
import pytest
import torch

from tests import mix_cases as mc
from tests.test_mix_host import CE_CASES, CLIP_CASES, NAN_CASES, TARGET_CASES, check_soft_ce
from x3dhip import mixing, mixops, ops

pytestmark = pytest.mark.gpu


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


@pytest.fixture()
def guard():
    _dev()
    prev = ops.set_guard(True)
    yield
    try:
        torch.cuda.synchronize()
        assert ops.check_guards() == []
    finally:
        ops.set_guard(prev)


def _offset_view(a, dev):
    """The array as a device tensor that starts one float into a larger buffer: its base is 4-byte aligned only.  Returns
    (view, buffer); the float before the view and the 7 after it are canaries."""
    buf = torch.full((a.size + 8,), 7.5, dtype=torch.float32, device=dev)
    assert buf.data_ptr() % 16 == 0
    v = buf[1:1 + a.size].view(a.shape)
    v.copy_(torch.from_numpy(a))
    return v, buf


def _canaries_intact(buf, n):
    return bool((buf[:1] == 7.5).all()) and bool((buf[1 + n:] == 7.5).all())


def _check_clips(x, plan, want, dev):
    dplan = mixops.plan_to_device(plan, dev)
    xd = torch.from_numpy(x).to(dev)
    got = mixops.mix_clips(xd, dplan)                                # fresh, guarded output
    assert torch.equal(got.cpu(), torch.from_numpy(want))
    xo, xbuf = _offset_view(x, dev)                                  # source and output one float off the 16-byte grid
    oo, obuf = _offset_view(np.zeros_like(x), dev)
    mixops.mix_clips(xo, dplan, out=oo)
    assert torch.equal(oo.cpu(), torch.from_numpy(want)) and _canaries_intact(obuf, x.size) and _canaries_intact(xbuf, x.size)
    o2, o2buf = _offset_view(np.zeros_like(x), dev)                  # aligned source, output off the grid
    mixops.mix_clips(xd, dplan, out=o2)
    assert torch.equal(o2.cpu(), torch.from_numpy(want)) and _canaries_intact(o2buf, x.size)
    got3 = mixops.mix_clips(xo, dplan)                               # source off the grid, aligned output
    assert torch.equal(got3.cpu(), torch.from_numpy(want))
    assert torch.equal(xd.cpu(), torch.from_numpy(x))                # the source is left alone


@pytest.mark.parametrize("shape", mc.CLIP_SHAPES, ids=str)
def test_mix_clips_equals_the_twin_on_every_case(shape, guard):
    dev = _dev()
    n = 0
    for name, x, plan in CLIP_CASES:
        if tuple(x.shape) == tuple(shape):
            _check_clips(x, plan, mixops.mix_clips_host(x, plan), dev)
            n += 1
    assert n >= 15


def test_mix_clips_nan_cases_bit_for_bit(guard):
    """CutMix is a select (no NaN of the partner outside the box, none of the sample inside it), lam == 1 is a bit copy."""
    dev = _dev()
    for name, x, plan, want in NAN_CASES:
        dplan = mixops.plan_to_device(plan, dev)
        for src in (torch.from_numpy(x).to(dev), _offset_view(x, dev)[0]):
            got = mixops.mix_clips(src, dplan).cpu().numpy()
            assert got.tobytes() == want.tobytes() == mixops.mix_clips_host(x, plan).tobytes(), name
            assert not np.isnan(got[0]).any() or name.startswith("nan-copy")


def test_mix_clips_big_batches(guard):
    """(8, 12, 64, 64): 96 runs of 4096 floats over 96 workgroups.  The clip kernel's grid is capped at 1024 workgroups (four
    per CU), so that case alone stays inside one pass of it; (5, 48, 136, 136) is 5 * 217 = 1085 runs, more than the cap: the
    workgroups 0..60 take a second run, in another sample.  Both with a copy, a mixup and a CutMix sample, aligned and one
    float off."""
    dev = _dev()
    for shape, seed in ((mc.BIG_SHAPE, 31), ((5, 48, 136, 136), 32)):
        B, P, H, W = shape
        assert shape == mc.BIG_SHAPE or B * -(-(P * H * W // 4) // 1024) > 1024
        x = mc.normals(shape, seed)
        plan = mc.plans(B, H, W)["modes_by_sample"]
        plan["y0"], plan["x0"] = np.where(plan["y1"] > 0, 3, 0), np.where(plan["x1"] > 0, 5, 0)
        want = torch.from_numpy(mixops.mix_clips_host(x, plan))
        dplan = mixops.plan_to_device(plan, dev)
        xd = torch.from_numpy(x).to(dev)
        assert torch.equal(mixops.mix_clips(xd, dplan).cpu(), want)
        oo, obuf = _offset_view(np.zeros(shape, np.float32), dev)
        mixops.mix_clips(xd, dplan, out=oo)
        assert torch.equal(oo.cpu(), want) and _canaries_intact(obuf, x.size)


def test_mix_clips_refusals_launch_nothing():
    dev = _dev()
    x = torch.from_numpy(mc.normals((2, 3, 4, 8, 8), 41)).to(dev)
    plan = mixops.plan_to_device(mixops.identity_plan(2), dev)
    buf = torch.zeros(2 * x.numel(), device=dev)
    buf[:x.numel()].copy_(x.view(-1))
    src = buf[:x.numel()].view(x.shape)
    before = buf.clone()
    for out in (src, buf[x.numel() // 2:x.numel() // 2 + x.numel()].view(x.shape), buf[4:4 + x.numel()].view(x.shape)):
        with pytest.raises(ValueError):
            mixops.mix_clips(src, plan, out=out)                     # in place, overlapping by half, overlapping by all but 4
    for bad in (dict(out=torch.zeros(2, 3, 4, 8, 9, device=dev)), dict(out=torch.zeros(x.shape)),
                dict(out=torch.zeros(x.shape, device=dev, dtype=torch.float64))):
        with pytest.raises(ValueError):
            mixops.mix_clips(src, plan, **bad)
    for bad_plan in (plan[:1], plan.cpu(), plan.to(torch.int8), torch.zeros(2, 33, dtype=torch.uint8, device=dev)[:, :32]):
        with pytest.raises(ValueError):
            mixops.mix_clips(src, bad_plan)
    with pytest.raises(ValueError):
        mixops.mix_clips(x.transpose(3, 4), plan)                    # not contiguous
    with pytest.raises(ValueError):
        mixops.mix_targets(torch.zeros(2, dtype=torch.int64, device=dev), plan, 400, smoothing=1.0)
    with pytest.raises(ValueError):
        mixops.mix_targets(torch.zeros(3, dtype=torch.int64, device=dev), plan, 400)
    with pytest.raises(ValueError):
        mixops.mix_targets(torch.zeros(2, 2, dtype=torch.int64, device=dev), plan, 400)
    torch.cuda.synchronize()
    assert torch.equal(buf, before)


def test_mix_targets_equals_the_twin_on_every_case(guard):
    dev = _dev()
    for name, labels, plan, C, sm in TARGET_CASES:
        want = torch.from_numpy(mixops.mix_targets_host(labels, plan, C, sm))
        dplan = mixops.plan_to_device(plan, dev)
        yd = torch.from_numpy(labels).to(dev)
        assert torch.equal(mixops.mix_targets(yd, dplan, C, sm).cpu(), want), name
        assert torch.equal(mixops.mix_targets(yd.view(-1, 1), dplan, C, sm).cpu(), want), name
        oo, obuf = _offset_view(np.zeros((labels.size, C), np.float32), dev)
        mixops.mix_targets(yd, dplan, C, sm, out=oo)
        assert torch.equal(oo.cpu(), want) and _canaries_intact(obuf, labels.size * C), name


def test_soft_ce_matches_torch_fp64_and_is_reproducible(guard):
    """The host test's inputs and bounds; two calls give the same bits."""
    dev = _dev()
    for name, z, t, gs in CE_CASES:
        zd, td = torch.from_numpy(z).to(dev), torch.from_numpy(t).to(dev)
        loss, dlog = mixops.soft_ce(zd, td, gs)
        loss2, dlog2 = mixops.soft_ce(zd, td, gs)
        check_soft_ce(float(loss), dlog.cpu().numpy(), z, t, gs)
        assert torch.equal(loss, loss2) and torch.equal(dlog, dlog2), name


def test_soft_ce_one_hot_targets_against_head_ce(guard):
    """soft_ce on exact one-hot rows against x3d_head_ce on the labels: the loss and the gradient within the bounds both are
    held to against fp64 (whether the BITS agree is recorded in profiles/mix/README.md, not required: the two gradient
    expressions differ)."""
    dev = _dev()
    R, C = 8, 400
    z = mc.ce_logits(R, C, 901)
    y = np.random.default_rng(902).integers(0, C, size=R)
    t = np.zeros((R, C), np.float32)
    t[np.arange(R), y] = 1.0
    zd = torch.from_numpy(z).to(dev)
    loss, dlog = mixops.soft_ce(zd, torch.from_numpy(t).to(dev))
    hl, hd = ops.head_ce(zd, torch.from_numpy(y).to(dev))
    print("soft_ce one-hot vs head_ce: loss bits equal %s, gradient bits equal %s" % (torch.equal(loss, hl), torch.equal(dlog, hd)))
    assert abs(float(loss) - float(hl)) <= 4e-6 * abs(float(hl))
    assert float((dlog - hd).abs().max()) <= 4e-6 * float(hd.abs().max())


def test_soft_ce_advances_the_draw_counter_by_one():
    dev = _dev()
    z, t = torch.from_numpy(mc.ce_logits(3, 157, 911)).to(dev), torch.from_numpy(mc.ce_targets(3, 157, 0.3, 0.1, 912)).to(dev)
    rng = ops.head_rng_state(dev, seed=77)
    before = rng.clone()
    a = mixops.soft_ce(z, t, 1.0, rng)
    b = mixops.soft_ce(z, t, 1.0)
    torch.cuda.synchronize()
    assert int(rng[0]) == int(before[0]) and int(rng[1]) == int(before[1]) + 1
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    for bad in ((z, t.double()), (z, t[:, :5]), (z, t.cpu()), (z[0], t[0]), (z, t, float("nan")), (z, t, 1.0, rng[:1])):
        with pytest.raises(ValueError):
            mixops.soft_ce(*bad)


def test_batch_mixer_on_the_device(guard):
    """The mixer's output is the twins' on its own plan; out= writes into the given tensors; both alphas 0 returns x itself."""
    dev = _dev()
    x = torch.from_numpy(mc.normals((4, 3, 4, 16, 16), 51)).to(dev)
    y = torch.tensor([[3], [399], [0], [17]], device=dev)
    m = mixing.BatchMixer(400, mixup_alpha=0.8, cutmix_alpha=1.0, label_smoothing=0.1, per_sample=True, seed=9)
    sx, sy = torch.zeros_like(x), torch.zeros(4, 400, device=dev)
    for k in range(6):
        out = (sx, sy) if k % 2 else None
        mx, st = m(x, y, out=out)
        plan = m.last_plan
        if out is not None:
            assert mx is sx and st is sy
        assert torch.equal(mx.cpu(), torch.from_numpy(mixops.mix_clips_host(x.cpu().numpy(), plan)))
        assert torch.equal(st.cpu(), torch.from_numpy(mixops.mix_targets_host(y.cpu().numpy(), plan, 400, 0.1)))
        assert torch.allclose(st.sum(1).cpu(), torch.ones(4), atol=1e-5)
    m0 = mixing.BatchMixer(400, label_smoothing=0.1)
    mx, st = m0(x, y)
    assert mx is x and st.shape == (4, 400)
    with pytest.raises(ValueError):
        m(x, y.float())
    with pytest.raises(ValueError):
        m(x, y[:3])
