"""Device-resident APMeter on the GPU (csrc_eval/apmeter.hip through x3dhip/evalops.py and apmeter.py): against the
reference's golden values, against the fp64 restatement (tests/apmeter_ref.py) on the meter's own stored rows (ties,
+-0.0, NaN, weights, sizes across tiles and passes, capacity growth), the crop-max and per-frame appends against torch,
graph capture, the sticky flags, determinism, and the Charades validation phases end to end."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import x3d_oracle as xo
from tests import apmeter_ref
from tests.test_apmeter_host import golden_cases
from x3dhip import synthetic

pytestmark = pytest.mark.gpu

NC = 157


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


def _meter():
    from apmeter import APMeter
    return APMeter()


def _ulp_close(a, b, ulps=2):
    a, b = a.detach().float().cpu().contiguous(), b.detach().float().cpu().contiguous()
    ia = a.view(torch.int32).long()
    ib = b.view(torch.int32).long()
    ia = torch.where(ia < 0, -(ia & 0x7fffffff), ia)
    ib = torch.where(ib < 0, -(ib & 0x7fffffff), ib)
    return bool(((ia - ib).abs() <= ulps).all())


def _restated(m):
    w = m.weights
    return apmeter_ref.average_precision(m.scores.numpy(), m.targets.numpy(), w.numpy() if w.numel() else None)


# --------------------------------------------------------------------------- golden
def test_meter_matches_reference_golden():
    dev = _dev()
    for name, (adds, ap, extra) in golden_cases().items():
        m = _meter()
        for i, a in enumerate(adds):
            if name == "cls_crops":
                m.add_logits(torch.from_numpy(a["logits"]).to(dev), torch.from_numpy(a["targets"]).float().to(dev),
                             n_crops=extra["n_crops"])
            elif name == "loc_frames":
                m.add_frames(torch.from_numpy(a["logits"]).to(dev), torch.from_numpy(a["labels"]).float().to(dev),
                             torch.from_numpy(a["masks"]).to(dev))
            elif i % 2 == 0:                               # host inputs, as the reference scripts pass them
                m.add(a["scores"], a["targets"].astype(np.int64), a.get("weights"))
            else:                                          # device inputs
                w = a.get("weights")
                m.add(torch.from_numpy(a["scores"]).to(dev), torch.from_numpy(a["targets"]).to(dev),
                      None if w is None else torch.from_numpy(w).to(dev))
        got = m.value()
        assert got.dtype == torch.float32 and got.shape == ap.shape, name
        np.testing.assert_allclose(got.numpy(), ap, rtol=0, atol=2e-6, err_msg=name)


# --------------------------------------------------------------------------- restatement on the stored rows
def _case(kind, N, K, seed):
    g = np.random.default_rng(seed)
    if kind == "random":
        s = g.random((N, K), dtype=np.float32)
    elif kind == "five_values":
        s = g.choice(np.array([0.1, 0.25, 0.5, 0.75, 0.9], np.float32), size=(N, K))
    elif kind == "zero_one":
        s = g.choice(np.array([0.0, 1.0], np.float32), size=(N, K))
    else:                                                  # "special": +-0.0, NaN, +-inf and a few values
        s = g.choice(np.array([0.0, -0.0, np.nan, np.inf, -np.inf, 0.5, -0.5, 1e-30], np.float32), size=(N, K))
    y = (g.random((N, K)) < 0.3).astype(np.int64)
    w = (g.random(N) * 2).astype(np.float32)
    w[g.random(N) < 0.1] = 0.0
    return s, y, w


@pytest.mark.parametrize("kind", ["random", "five_values", "zero_one", "special"])
@pytest.mark.parametrize("weighted", [False, True])
def test_meter_matches_restatement_with_ties(kind, weighted):
    dev = _dev()
    s, y, w = _case(kind, 3001, 9, seed=2 * ["random", "five_values", "zero_one", "special"].index(kind) + int(weighted))
    m = _meter()
    for lo, hi in ((0, 1000), (1000, 1001), (1001, 3001)):
        m.add(torch.from_numpy(s[lo:hi]).to(dev), torch.from_numpy(y[lo:hi]).to(dev),
              torch.from_numpy(w[lo:hi]).to(dev) if weighted else None)
    got = m.value().double().numpy()
    assert torch.equal(m.scores.view(torch.int32), torch.from_numpy(s).view(torch.int32))
    ref = apmeter_ref.average_precision(s, y, w if weighted else None)
    np.testing.assert_allclose(got, ref, rtol=0, atol=1e-6)
    np.testing.assert_allclose(got, _restated(m), rtol=0, atol=1e-6)


@pytest.mark.parametrize("N", [1, 63, 64, 65, 4095, 4097, (1 << 20) + 3])
def test_meter_sizes_across_tiles_and_passes(N):
    dev = _dev()
    K = 3 if N > 5000 else 11
    g = torch.Generator(device="cpu").manual_seed(N)
    s = torch.rand((N, K), generator=g)
    s[:, 1] = torch.floor(s[:, 1] * 7) / 7                  # ties
    s[:, 2] = 0.5 + torch.rand(N, generator=g) * 1e-3       # shared high bits: skipped passes
    y = (torch.rand((N, K), generator=g) < 0.2).long()
    m = _meter()
    m.add(s.to(dev), y.to(dev))
    got = m.value().double().numpy()
    np.testing.assert_allclose(got, apmeter_ref.average_precision(s.numpy(), y.numpy()), rtol=0, atol=1e-6)


def test_meter_grows_across_adds():
    dev = _dev()
    m = _meter()
    caps = set()
    S, Y = [], []
    for i in range(6):
        s, y, _ = _case("five_values", 700, 5, seed=i)
        m.add(torch.from_numpy(s).to(dev), torch.from_numpy(y).to(dev))
        caps.add(m._cap)
        S.append(s)
        Y.append(y)
    assert len(caps) >= 2                                   # the capacity grew at least once
    got = m.value().double().numpy()
    np.testing.assert_allclose(got, apmeter_ref.average_precision(np.concatenate(S), np.concatenate(Y)), rtol=0, atol=1e-6)


# --------------------------------------------------------------------------- appends vs torch
def test_add_logits_rows_and_max_logits():
    dev = _dev()
    b, n, K = 5, 10, NC
    g = torch.Generator(device="cpu").manual_seed(3)
    z = (torch.randn((b * n, K), generator=g) * 6).to(dev)
    y = (torch.rand((b, K), generator=g) < 0.1).float().to(dev)
    m = _meter()
    mx = m.add_logits(z.view(b * n, K, 1), y, n_crops=n)
    ref_p = torch.sigmoid(z).view(b, n, K).amax(1)
    assert torch.equal(mx, z.view(b, n, K).amax(1))
    assert _ulp_close(m.scores, ref_p.cpu())
    assert torch.equal(m.targets, y.long().cpu())
    m2 = _meter()                                           # n_crops = 1: the training rows
    mx2 = m2.add_logits(z, (torch.rand((b * n, K), generator=g) < 0.1).float().to(dev))
    assert torch.equal(mx2, z) and _ulp_close(m2.scores, torch.sigmoid(z).cpu())


def test_add_frames_rows_and_order():
    dev = _dev()
    B, K, T, TL = 4, NC, 8, 21
    g = torch.Generator(device="cpu").manual_seed(5)
    z = (torch.randn((B, K, T), generator=g) * 3).to(dev)
    y = (torch.rand((B, K, TL), generator=g) < 0.1).float().to(dev)
    masks = torch.zeros(B, TL)
    masks[0, :TL] = 1
    masks[1, :13] = 1
    masks[1, 4] = 0                                          # a zero inside the valid prefix (valid_t = 12)
    masks[2, :] = 0                                          # valid_t = 0
    masks[3, :5] = 1
    masks = masks.to(dev)
    m = _meter()
    m.add_frames(z, y, masks)
    # the reference's per-sample slicing (train_x3d_charades_loc.py:165-186) in torch ops
    pfl = F.interpolate(z, TL, mode='linear')
    probs = torch.sigmoid(pfl) * masks.unsqueeze(1)
    valid_t = torch.sum(masks, dim=1).int()
    rows = torch.cat([probs[b][:, :valid_t[b].item()].transpose(0, 1) for b in range(B)], 0)
    labs = torch.cat([y[b][:, :valid_t[b].item()].transpose(0, 1) for b in range(B)], 0)
    assert m.scores.shape == rows.shape == (21 + 12 + 0 + 5, K)
    assert _ulp_close(m.scores, rows.cpu())
    assert torch.equal(m.targets, labs.long().cpu())
    np.testing.assert_allclose(m.value().double().numpy(), _restated(m), rtol=0, atol=1e-6)


# --------------------------------------------------------------------------- graph capture
def _inputs(dev, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    b, n, B, K, T, TL = 3, 2, 2, 7, 4, 9
    z = (torch.randn((b * n, K), generator=g) * 4).to(dev)
    y = (torch.rand((b, K), generator=g) < 0.3).float().to(dev)
    pf = (torch.randn((B, K, T), generator=g) * 4).to(dev)
    lab = (torch.rand((B, K, TL), generator=g) < 0.3).float().to(dev)
    masks = torch.ones(B, TL, device=dev)
    return z, y, pf, lab, masks, n, b + B * TL


def test_graph_replays_equal_eager_and_overflow_raises():
    dev = _dev()
    z, y, pf, lab, masks, n, per = _inputs(dev, 11)
    R = 5
    eager = _meter()
    for _ in range(R):
        eager.add_logits(z, y, n_crops=n)
        eager.add_frames(pf, lab, masks)
    m = _meter()
    m.add_logits(z, y, n_crops=n)                            # eager first add: the buffers exist before the capture
    m.add_frames(pf, lab, masks)
    m.reserve(R * per)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        with torch.cuda.graph(graph, stream=s):
            m.add_logits(z, y, n_crops=n)
            m.add_frames(pf, lab, masks)
    torch.cuda.current_stream().wait_stream(s)
    for _ in range(R - 1):
        graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(m.scores.view(torch.int32), eager.scores.view(torch.int32))
    assert torch.equal(m.targets, eager.targets)
    assert torch.equal(m.value().view(torch.int32), eager.value().view(torch.int32))
    # replaying past the reserved capacity: the append writes nothing, the sticky flag makes value() raise
    for _ in range((m._cap - R * per) // per + 1):
        graph.replay()
    torch.cuda.synchronize()
    assert m.scores.shape[0] <= m._cap
    assert torch.isnan(m.value_device()).all()
    with pytest.raises(RuntimeError, match="reserve"):
        m.value()


def test_growth_inside_capture_raises():
    dev = _dev()
    z, y, pf, lab, masks, n, per = _inputs(dev, 12)
    m = _meter()
    m.add_logits(z, y, n_crops=n)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    big = torch.zeros((m._cap * 2, z.shape[1]), device=dev)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with pytest.raises(RuntimeError, match="reserve"):
        with torch.cuda.stream(s):
            with torch.cuda.graph(graph, stream=s):
                m.add_logits(big, torch.zeros((big.shape[0], z.shape[1]), device=dev))
    torch.cuda.synchronize()


# --------------------------------------------------------------------------- flags, determinism
def test_flags_make_value_raise():
    dev = _dev()
    m = _meter()
    m.add(torch.rand(10, 3, device=dev), torch.tensor([[0, 1, 2]] * 10, device=dev))
    with pytest.raises(ValueError, match="0 / 1"):
        m.value()
    m = _meter()
    w = torch.ones(10, device=dev)
    w[4] = -1.0
    m.add(torch.rand(10, 3, device=dev), torch.zeros(10, 3, device=dev), w)
    with pytest.raises(ValueError, match="negative"):
        m.value()
    m.reset()                                               # reset clears the flags
    m.add(torch.rand(10, 3, device=dev), torch.ones(10, 3, device=dev))
    assert torch.equal(m.value(), torch.ones(3))


def test_value_is_deterministic():
    dev = _dev()
    s, y, w = _case("five_values", 50000, 13, seed=9)
    out = []
    for _ in range(2):
        m = _meter()
        m.add(torch.from_numpy(s).to(dev), torch.from_numpy(y).to(dev), torch.from_numpy(w).to(dev))
        out.append(m.value())
        out.append(m.value())
    for o in out[1:]:
        assert torch.equal(o.view(torch.int32), out[0].view(torch.int32))


# --------------------------------------------------------------------------- end to end
def _model(dev, task, seed=0):
    import x3d
    net = x3d.generate_model("S", n_classes=NC, dropout=0.0, base_bn_splits=1, task=task)
    net.load_state_dict(synthetic.procedural_state_dict(xo.state_template("S", NC, 1), seed))
    return net.to(dev)


def test_validate_cls_and_loc_match_torch_and_restatement():
    import charades_eval
    dev = _dev()
    b, n, T, H = 2, 3, 4, 64
    batches = []
    for i in range(2):
        x = synthetic.synthetic_clips(b * n, T, H, H, seed=100 + i).view(b, n, 3, T, H, H).to(dev)
        y = (torch.rand((b, NC), generator=torch.Generator().manual_seed(i)) < 0.1).float().to(dev)
        batches.append((x, y))
    net = _model(dev, "class")
    res = charades_eval.validate_cls(net, batches)
    with torch.no_grad():
        P, Y, L = [], [], []
        for x, y in batches:
            lg = net(x.view(b * n, 3, T, H, H)).squeeze(2).view(b, n, NC)
            P.append(torch.sigmoid(lg).amax(1))
            Y.append(y)
            L.append(F.binary_cross_entropy_with_logits(lg.amax(1), y))
    ap = apmeter_ref.average_precision(torch.cat(P).cpu().numpy(), torch.cat(Y).cpu().numpy())
    np.testing.assert_allclose(res["ap"].double().numpy(), ap, rtol=0, atol=1e-6)
    assert abs(res["map"] - float(res["ap"].mean())) < 1e-7 and res["rows"] == 2 * b
    assert abs(res["cls_loss"] - float(sum(L) / 2)) <= 1e-5 * abs(res["cls_loss"])

    B, TL = 2, 11
    lb = []
    for i in range(2):
        x = synthetic.synthetic_clips(B, T, H, H, seed=200 + i).to(dev)
        y = (torch.rand((B, NC, TL), generator=torch.Generator().manual_seed(10 + i)) < 0.1).float().to(dev)
        masks = torch.ones(B, TL, device=dev)
        masks[1, 7:] = 0
        lb.append((x, y, masks))
    net = _model(dev, "loc", seed=1)
    res = charades_eval.validate_loc(net, lb)
    with torch.no_grad():
        S, Y, C, Lo = [], [], [], []
        for x, y, masks in lb:
            pfl = F.interpolate(net(x), TL, mode='linear')
            probs = torch.sigmoid(pfl) * masks.unsqueeze(1)
            vt = masks.sum(1).int()
            for bb in range(B):
                S.append(probs[bb][:, :vt[bb].item()].t())
                Y.append(y[bb][:, :vt[bb].item()].t())
            C.append(F.binary_cross_entropy_with_logits(pfl.amax(2), y.amax(2)))
            Lo.append(F.binary_cross_entropy_with_logits(pfl, y))
    ap = apmeter_ref.average_precision(torch.cat(S).cpu().numpy(), torch.cat(Y).cpu().numpy())
    np.testing.assert_allclose(res["ap"].double().numpy(), ap, rtol=0, atol=1e-6)
    assert res["rows"] == 2 * (TL + 7)
    assert abs(res["cls_loss"] - float(sum(C) / 2)) <= 1e-5 * abs(res["cls_loss"])
    assert abs(res["loc_loss"] - float(sum(Lo) / 2)) <= 1e-5 * abs(res["loc_loss"])


def test_trainer_loc_graph_steps_feed_add_frames():
    from x3dhip.trainer import Trainer
    dev = _dev()
    net = _model(dev, "loc", seed=2).train(True)
    tr = Trainer(net, lr=0.01, momentum=0.9, weight_decay=1e-5, objective="loc", use_graph=True)
    m = _meter()
    B, T, H, TL = 2, 4, 64, 9
    S, Y = [], []
    for i in range(3):
        x = synthetic.synthetic_clips(B, T, H, H, seed=300 + i).to(dev)
        y = (torch.rand((B, NC, TL), generator=torch.Generator().manual_seed(20 + i)) < 0.1).float().to(dev)
        masks = torch.ones(B, TL, device=dev)
        masks[0, 6:] = 0
        _, logits = tr.train_step(x, y)
        m.add_frames(logits, y, masks)                      # same stream, before the next replay overwrites logits
        probs = torch.sigmoid(F.interpolate(logits, TL, mode='linear')) * masks.unsqueeze(1)
        S += [probs[0][:, :6].t().clone(), probs[1].t().clone()]
        Y += [y[0][:, :6].t(), y[1].t()]
    np.testing.assert_allclose(m.value().double().numpy(),
                               apmeter_ref.average_precision(torch.cat(S).cpu().numpy(), torch.cat(Y).cpu().numpy()),
                               rtol=0, atol=1e-6)


# --------------------------------------------------------------------------- captured graphs across growth / replacement
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


def _replay_retired(m, graph):
    """Replay a graph captured before the meter moved to new buffers: the state it appends to must be retired (capacity
    0) first, so that the replay writes nothing (checked before replaying)."""
    from x3dhip import _evallib
    torch.cuda.synchronize()
    assert m._retired, "the captured state was not retired"
    old_state = m._retired[-1][0]
    assert int(old_state[_evallib.S_CAPACITY].item()) == 0
    count = m._count()
    graph.replay()
    torch.cuda.synchronize()
    assert m._count() == count                              # nothing appended to the live meter
    assert int(old_state[_evallib.S_OVERFLOW].item()) == 1
    with pytest.raises(RuntimeError, match="capture again"):
        m.value()


@pytest.mark.parametrize("how", ["reserve", "eager_growth", "reset_other_k"])
def test_graph_captured_before_the_buffers_move_appends_nothing(how):
    dev = _dev()
    z, y, pf, lab, masks, n, per = _inputs(dev, 13)
    m = _meter()
    m.add_logits(z, y, n_crops=n)
    m.add_frames(pf, lab, masks)
    graph = _capture(m, z, y, pf, lab, masks, n)
    graph.replay()
    if how == "reserve":
        m.reserve(4 * m._cap)
    elif how == "eager_growth":
        m.add(torch.rand((m._cap, z.shape[1]), device=dev), torch.zeros((m._cap, z.shape[1]), device=dev))
    else:
        m.reset()
        m.add(torch.rand((5, 3), device=dev), torch.ones((5, 3), device=dev))
    rows_before = m.scores.clone()
    _replay_retired(m, graph)
    assert torch.equal(m.scores.view(torch.int32), rows_before.view(torch.int32))
    if how == "reserve":                                    # rows appended before the growth are kept
        eager = _meter()
        for _ in range(2):                                  # the eager add and the replay before the growth
            eager.add_logits(z, y, n_crops=n)
            eager.add_frames(pf, lab, masks)
        assert torch.equal(m.scores.view(torch.int32), eager.scores.view(torch.int32))
    m.reset()                                               # reset clears the report; a new capture appends again
    m.add_logits(z, y, n_crops=n)
    m.add_frames(pf, lab, masks)
    m.reserve(m._count() + 10 * per)
    graph2 = _capture(m, z, y, pf, lab, masks, n)
    graph2.replay()
    torch.cuda.synchronize()
    assert torch.is_tensor(m.value())


def test_graph_keeps_its_row_offsets_when_a_larger_batch_arrives():
    dev = _dev()
    z, y, pf, lab, masks, n, per = _inputs(dev, 14)
    big_pf = pf.repeat(40, 1, 1)                            # B = 80 > the 64 row offsets of a fresh meter
    big_lab, big_masks = lab.repeat(40, 1, 1), masks.repeat(40, 1)
    eager, m = _meter(), _meter()
    for mm in (eager, m):
        mm.reserve(100000)
        mm.add_logits(z, y, n_crops=n)
        mm.add_frames(pf, lab, masks)
    graph = _capture(m, z, y, pf, lab, masks, n)
    m.add_frames(big_pf, big_lab, big_masks)               # eager: a larger row-offset scratch
    graph.replay()
    eager.add_frames(big_pf, big_lab, big_masks)
    eager.add_logits(z, y, n_crops=n)
    eager.add_frames(pf, lab, masks)
    torch.cuda.synchronize()
    assert not m._retired
    assert torch.equal(m.scores.view(torch.int32), eager.scores.view(torch.int32))
    assert torch.equal(m.value().view(torch.int32), eager.value().view(torch.int32))


# --------------------------------------------------------------------------- class batching of value()
def test_value_with_fewer_workspace_slots_than_classes():
    from x3dhip import evalops
    dev = _dev()
    s, y, w = _case("five_values", 5000, 13, seed=21)
    m = _meter()
    m.add(torch.from_numpy(s).to(dev), torch.from_numpy(y).to(dev), torch.from_numpy(w).to(dev))
    full = m.value_device()
    slot = 16 * ((m._cap + 63) // 64 * 64)
    for slots in (1, 2, 5):                                 # 13 classes take turns on 1, 2 or 5 workspace slots
        ws = torch.empty(slots * slot, dtype=torch.uint8, device=dev)
        got = evalops.ap_value(m._state, m._scores, m._targets, m._weights, workspace=ws)
        assert torch.equal(got.view(torch.int32), full.view(torch.int32)), slots
    np.testing.assert_allclose(full.double().cpu().numpy(), apmeter_ref.average_precision(s, y, w), rtol=0, atol=1e-6)


def test_value_at_a_million_rows_and_157_classes_batches_the_classes():
    """2^20 rows x 157 classes: the default workspace holds 128 class slots under its cap, so the classes take two turns;
    bitwise equal to a workspace with a slot per class, and classes of both turns against the restatement."""
    from x3dhip import evalops
    dev = _dev()
    N, K = 1 << 20, NC
    g = torch.Generator(device=dev).manual_seed(77)
    s = torch.sigmoid(torch.randn((N, K), device=dev, generator=g) * 3)
    y = (torch.rand((N, K), device=dev, generator=g) < 0.05).float()
    m = _meter()
    m.add(s, y)
    assert evalops.ap_workspace_bytes(K, m._cap) < K * 16 * m._cap
    batched = m.value_device()
    ws = torch.empty(K * 16 * ((m._cap + 63) // 64 * 64), dtype=torch.uint8, device=dev)
    one_turn = evalops.ap_value(m._state, m._scores, m._targets, None, workspace=ws)
    assert torch.equal(batched.view(torch.int32), one_turn.view(torch.int32))
    del ws
    cols = [0, 127, 128, 156]
    ref = apmeter_ref.average_precision(s[:, cols].cpu().numpy(), y[:, cols].cpu().numpy().astype(np.int64))
    np.testing.assert_allclose(batched[cols].double().cpu().numpy(), ref, rtol=0, atol=1e-6)


# --------------------------------------------------------------------------- per-frame interpolation, bit for bit
@pytest.mark.parametrize("T,TL", [(8, 21), (4, 9), (32, 160), (16, 16), (8, 5)])
def test_add_frames_interpolates_as_f_interpolate_bitwise(T, TL):
    """Rows of add_frames (masks 1) == the crop kernel's sigmoid of torch's own F.interpolate output, bit for bit: both
    appends share the device sigmoid, so the per-frame kernel's interpolation equals F.interpolate's exactly (torch's CPU
    result: its source index and value are fused multiply-adds)."""
    dev = _dev()
    B, K = 3, NC
    g = torch.Generator(device="cpu").manual_seed(T * 1000 + TL)
    z = torch.randn((B, K, T), generator=g) * 4
    y = (torch.rand((B, K, TL), generator=g) < 0.1).float()
    frames, logits = _meter(), _meter()
    frames.add_frames(z.to(dev), y.to(dev), torch.ones(B, TL, device=dev))
    zi = F.interpolate(z, TL, mode='linear').permute(0, 2, 1).reshape(B * TL, K).contiguous()
    assert torch.equal(torch.from_numpy(apmeter_ref.interp_linear(z.numpy(), TL)).permute(0, 2, 1).reshape(B * TL, K), zi)
    logits.add_logits(zi.to(dev), y.permute(0, 2, 1).reshape(B * TL, K).contiguous().to(dev))
    assert torch.equal(frames.scores.view(torch.int32), logits.scores.view(torch.int32))
    assert torch.equal(frames.targets, logits.targets)
