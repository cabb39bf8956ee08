"""JPEG decoder on the GPU (libx3djpeg.so through x3dhip.jpegops): every golden of tests/golden/jpeg_cases.npz equal to
Pillow's decode bit for bit (torch.equal, no tolerance), alone, in one mixed batch and into strided destinations with
guard bytes; the two kernels alone against tests/jpeg_ref.py; rejects; FolderKinetics against DeviceVideoKinetics on the
same video; one training step from a frame folder.  Only the committed fixture is read: Pillow is not needed."""
import math
import os
import random

import numpy as np
import pytest
import torch

import frames
from kinetics_multigrid import DeviceVideoKinetics
from tests import jpeg_ref as jr
from x3dhip import _jpeglib, jpegops
from x3dhip._lib import X3DHipError, stream

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
CASES = jr.load_cases()
GOOD = {k: v for k, v in CASES.items() if v[1] is not None}
NAMES = list(GOOD)
VIDEO = [CASES["vid_%02d" % t] for t in range(12)]


@pytest.fixture(scope="module")
def dec():
    return jpegops.JpegDecoder(DEV, threads=4)


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def test_threads_are_clamped_and_the_device_must_be_a_gpu():
    assert jpegops.JpegDecoder(DEV, threads=0).threads == 1
    assert jpegops.JpegDecoder(DEV, threads=1000).threads == 16
    assert jpegops.JpegDecoder(DEV).threads == 8
    with pytest.raises(ValueError):
        jpegops.JpegDecoder("cpu")


@pytest.mark.parametrize("name", NAMES)
def test_decode_equals_pillow(dec, name):
    data, rgb = GOOD[name]
    out, = dec.decode([data])
    assert out.dtype == torch.uint8 and out.device == DEV and tuple(out.shape) == rgb.shape
    assert torch.equal(out, _t(rgb)), name


@pytest.mark.parametrize("name", NAMES)
def test_decode_into_a_strided_slot_leaves_the_guards_alone(dec, name):
    data, rgb = GOOD[name]
    H, W, _ = rgb.shape
    pitch = 3 * W + 16
    raw = torch.full((4, H, pitch), 0xA5, dtype=torch.uint8, device=DEV)   # guard frame, two slots, guard frame
    dst = raw.as_strided((2, H, W, 3), (H * pitch, pitch, 3, 1), H * pitch)
    assert dec.decode_into([data, data], dst) is dst
    want = _t(rgb)
    assert torch.equal(dst[0], want) and torch.equal(dst[1], want)
    assert bool((raw[0] == 0xA5).all()) and bool((raw[3] == 0xA5).all())
    assert bool((raw[1:3, :, 3 * W:] == 0xA5).all())


def test_decode_into_checks_sizes_and_strides(dec):
    data, rgb = GOOD["c420_37x53_q75"]
    H, W, _ = rgb.shape
    with pytest.raises(ValueError):
        dec.decode_into([data], torch.empty((1, H, W + 1, 3), dtype=torch.uint8, device=DEV))
    with pytest.raises(ValueError):
        dec.decode_into([data, data], torch.empty((1, H, W, 3), dtype=torch.uint8, device=DEV))
    with pytest.raises(ValueError):
        dec.decode_into([data], torch.empty((1, H, W, 3), dtype=torch.float32, device=DEV))
    with pytest.raises(ValueError):
        dec.decode_into([data], torch.empty((1, H, 3, W), dtype=torch.uint8, device=DEV).permute(0, 1, 3, 2))
    with pytest.raises(ValueError):
        dec.decode_into([data], torch.empty((1, H, W, 3), dtype=torch.uint8))


def test_one_call_decodes_all_goldens_of_mixed_size_and_subsampling(dec):
    outs = dec.decode([GOOD[n][0] for n in NAMES])
    assert len(outs) == len(NAMES)
    for n, o in zip(NAMES, outs):
        assert torch.equal(o, _t(GOOD[n][1])), n
        assert torch.equal(o, dec.decode([GOOD[n][0]])[0]), n


def _jobs(infos, coef, planes, dst, strides):
    jobs = np.zeros(len(infos), dtype=_jpeglib.FRAME_JOB_DT)
    jpegops.fill_jobs(jobs, infos)
    jobs["coef"], jobs["planes"], jobs["dst"], jobs["dst_stride"] = coef, planes, dst, strides
    return torch.from_numpy(jobs.view(np.uint8)).to(DEV)


def test_idct_entry_alone_gives_the_restatements_padded_planes():
    infos = np.zeros(len(NAMES), dtype=_jpeglib.INFO_DT)
    coefs, want = [], []
    for i, n in enumerate(NAMES):
        data = GOOD[n][0]
        rc, _, msg = _jpeglib.parse(data, infos[i:i + 1])
        assert rc == 0, msg
        _, c, p = jr.planes_of(data)
        coefs.append(np.concatenate([k.ravel() for k in c]))
        want.append(np.concatenate([k.ravel() for k in p]))
    offs = np.concatenate([[0], np.cumsum([c.size for c in coefs])])
    assert np.array_equal(offs[1:] - offs[:-1], infos["coef_count"])
    coef = _t(np.concatenate(coefs))
    planes = torch.full((int(offs[-1]) + 64,), 0xA5, dtype=torch.uint8, device=DEV)
    jd = _jobs(infos, coef.data_ptr() + 2 * offs[:-1], planes.data_ptr() + offs[:-1], 0, 0)
    _jpeglib.check(_jpeglib.lib().x3djpeg_idct(jd.data_ptr(), len(NAMES), int(infos["nblocks"].max()), stream()))
    got = planes.cpu().numpy()
    for i, n in enumerate(NAMES):
        assert np.array_equal(got[offs[i]:offs[i + 1]], want[i]), n
    assert np.all(got[offs[-1]:] == 0xA5)


@pytest.mark.parametrize("hv", [(1, 1), (2, 1), (2, 2)])
def test_to_rgb_entry_alone_on_random_planes(hv):
    """Uniform 0..255 planes, not JPEG derived: both clamps and every rounding branch of the upsampling are hit."""
    hs, vs = hv
    sizes = [(1, 1), (2, 3), (3, 4), (5, 6), (9, 17), (31, 33)]
    rng = np.random.default_rng(11 + 2 * hs + vs)
    infos = np.zeros(len(sizes), dtype=_jpeglib.INFO_DT)
    planes, want = [], []
    for i, (H, W) in enumerate(sizes):
        mx, my = -(-W // (8 * hs)), -(-H // (8 * vs))
        r = infos[i]
        r["width"], r["height"], r["ncomp"], r["hmax"], r["vmax"] = W, H, 3, hs, vs
        r["blocks_w"], r["blocks_h"] = (mx * hs, mx, mx), (my * vs, my, my)
        r["cw"], r["ch"] = (W, -(-W // hs), -(-W // hs)), (H, -(-H // vs), -(-H // vs))
        nb = r["blocks_w"].astype(np.int64) * r["blocks_h"]
        r["block_start"] = (0, nb[0], nb[0] + nb[1])
        r["nblocks"] = nb.sum()
        p = [rng.integers(0, 256, (int(r["blocks_h"][c]) * 8, int(r["blocks_w"][c]) * 8), dtype=np.uint8) for c in range(3)]
        planes.append(np.concatenate([k.ravel() for k in p]))
        want.append(jr.to_rgb(p, W, H, hs, vs))
    offs = np.concatenate([[0], np.cumsum([p.size for p in planes])])
    pl = _t(np.concatenate(planes))
    outs = [torch.full((H, W, 3), 0xA5, dtype=torch.uint8, device=DEV) for H, W in sizes]
    jd = _jobs(infos, 0, pl.data_ptr() + offs[:-1], [o.data_ptr() for o in outs], [3 * W for _, W in sizes])
    _jpeglib.check(_jpeglib.lib().x3djpeg_to_rgb(jd.data_ptr(), len(sizes), 33, 31, stream()))
    seen = set()
    for (H, W), o, w in zip(sizes, outs, want):
        assert torch.equal(o, _t(w)), (hv, H, W)
        seen |= {int(w.min()), int(w.max())}
    assert {0, 255} <= seen


def test_decode_on_a_side_stream_into_poisoned_output(dec):
    names = ["c420_120x90_q50", "c422_33x70_q60", "grey_30x44"]
    outs = [torch.full(GOOD[n][1].shape, 0xA5, dtype=torch.uint8, device=DEV) for n in names]
    torch.cuda.synchronize()
    s = torch.cuda.Stream(device=DEV)
    with torch.cuda.stream(s):
        got = dec.decode([GOOD[n][0] for n in names], out=outs)
    s.synchronize()
    for n, o, g in zip(names, outs, got):
        assert g is o and torch.equal(o, _t(GOOD[n][1])), n


@pytest.mark.parametrize("bad", ["reject_progressive", "reject_cmyk", "reject_truncated"])
def test_a_reject_inside_a_batch_names_its_index_and_launches_nothing(dec, bad):
    good = GOOD["c420_37x53_q75"]
    outs = [torch.full(good[1].shape, 0xA5, dtype=torch.uint8, device=DEV) for _ in range(3)]
    with pytest.raises(X3DHipError, match=r"frame 1 of the batch.*(progressive|4 components|scan data ends)"):
        dec.decode([good[0], CASES[bad][0], good[0]], out=outs)
    torch.cuda.synchronize()
    assert all(bool((o == 0xA5).all()) for o in outs)
    assert torch.equal(dec.decode([good[0]])[0], _t(good[1]))            # the decoder is still usable


def _folder(tmp_path):
    path = str(tmp_path / "video")
    os.makedirs(path)
    for t, (data, _) in enumerate(VIDEO):
        with open(os.path.join(path, frames.FRAME_NAME.format(t + 1)), "wb") as f:
            f.write(data)
    return path


def test_decode_folder_equals_pillow(tmp_path):
    v = frames.decode_folder(_folder(tmp_path), DEV, threads=2, chunk=5)
    assert torch.equal(v, _t(np.stack([rgb for _, rgb in VIDEO])))


def test_folder_kinetics_equals_device_video_kinetics(tmp_path):
    path = _folder(tmp_path)
    whole = _t(np.stack([rgb for _, rgb in VIDEO]))
    kw = dict(sample_duration=8, gamma_tau=2, crop_size=32, x3d_version='M')
    a = frames.FolderKinetics([path, path], [3, 5], rng=random.Random(99), device=DEV, threads=2, **kw)
    b = DeviceVideoKinetics([whole, whole], [3, 5], rng=random.Random(99), **kw)
    assert len(a) == len(b) == 2
    for iteration, long_state in ((0, 3), (1, 3), (2, 2), (1, 0)):
        ca, ya, la, sa = a.batch([0, 1, 1], iteration, long_state)
        cb, yb, lb, sb = b.batch([0, 1, 1], iteration, long_state)
        assert ca.shape == cb.shape and ca.dtype == torch.float32 and torch.equal(ca, cb), (iteration, long_state)
        assert torch.equal(ya, yb) and la == lb and sa == sb
    out = torch.empty_like(ca)
    assert a.batch([1, 0, 1], 1, 0, out=out)[0] is out
    va, ya = a.val_batch([0, 1], crops=3, sample_duration=10)
    vb, yb = b.val_batch([0, 1], crops=3, sample_duration=10)
    assert tuple(va.shape) == (2, 3, 3, 5, 32, 32) and torch.equal(va, vb) and torch.equal(ya, yb)


def test_one_training_step_from_a_frame_folder(tmp_path, capsys):
    import train_x3d_kinetics_multigrid as tk
    ds = frames.FolderKinetics([_folder(tmp_path)], [7], sample_duration=80, gamma_tau=5, crop_size=32,
                               rng=random.Random(1), device=DEV, threads=2)
    steps, rate = tk.run(batch_size=2, max_steps_run=1, iterations_per_epoch=40, max_epochs=3, save_every=0,
                         use_graph=False, log_every=1, frames_root=ds)
    assert steps == 1 and rate > 0
    line, = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith(" step 1 ")]
    loss = float(line.split(" loss ")[1].split()[0])
    assert math.isfinite(loss) and 0 < loss < 20, line
