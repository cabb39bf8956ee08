"""The parallel Huffman decoder on the GPU (x3djpeg_entropy_decode_batch, JpegDecoder(entropy="device")): coefficients equal
to the host decoder's bit for bit (torch.equal) for every good case of both fixture files at three subsequence lengths,
alone and in one mixed batch, inside 0x5A5A guards; pixels equal to Pillow's goldens and to the host path; damaged
streams (only ones the sanitised CPU run of tests/test_jpeg_entropy_host.py has been through) fail their own frame and
nothing else; a captured batch replays to the eager result; FolderKinetics reads the same clips either way."""
import os
import random

import numpy as np
import pytest
import torch

import frames
from tests import jpeg_entropy_cases as jc
from tests import jpeg_ref as jr
from x3dhip import _jpeglib, jpegops
from x3dhip._lib import X3DHipError, stream

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
OLD = jr.load_cases()
NEW = jc.load_entropy_cases()
GOOD = jc.good_cases()
NAMES = list(GOOD)
GUARD = 64          # int16 elements on either side of the whole coefficient buffer
_HOST = {}


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _host_coef(data):
    """(rc, info, int16 coefficients) of the host decoder, computed once per file."""
    if data not in _HOST:
        rc, info, msg = _jpeglib.parse(data)
        assert rc == 0, msg
        coef = np.zeros(int(info["coef_count"][0]), np.int16)
        rc, _ = _jpeglib.entropy_decode(data, info, coef.ctypes.data, coef.nbytes)
        _HOST[data] = (rc, info, coef)
    return _HOST[data]


def _device_coefs(datas, sub_bits):
    """x3djpeg_entropy_decode_batch alone on a batch.  Returns (status as numpy, per frame int16 tensors, rounds per frame);
    asserts that the guards around the coefficient buffer are intact."""
    n = len(datas)
    infos = np.zeros(n, _jpeglib.INFO_DT)
    blob, scan_at, seg_at, scan_bytes, nseg, ws = bytearray(), [], [], [], [], []
    for i, d in enumerate(datas):
        rc, info, msg = _jpeglib.parse(d, infos[i:i + 1])
        assert rc == 0, msg
        rc, scan, segs, msg = _jpeglib.scan_prepare(d, infos[i:i + 1])
        assert rc == 0, msg
        for part, at in ((scan.tobytes(), scan_at), (segs.tobytes(), seg_at)):
            blob += b"\0" * (-len(blob) % 16)
            at.append(len(blob))
            blob += part
        scan_bytes.append(scan.size - _jpeglib.SCAN_PAD)
        nseg.append(segs.size)
        ws.append(_jpeglib.workspace_bytes(scan_bytes[-1], nseg[-1], sub_bits))
    dev_bytes = _t(np.frombuffer(bytes(blob), np.uint8))
    counts = infos["coef_count"].astype(np.int64)
    offs = np.concatenate([[0], np.cumsum(counts)])
    total = int(offs[-1])
    coef = torch.full((total + 2 * GUARD,), 0x5A5A, dtype=torch.int16, device=DEV)
    ws_off = np.concatenate([[0], np.cumsum(ws)])
    workspace = torch.zeros(int(ws_off[-1]), dtype=torch.uint8, device=DEV)
    status = torch.full((n,), 77, dtype=torch.int32, device=DEV)
    sj = np.zeros(n, _jpeglib.SCAN_JOB_DT)
    _jpeglib.fill_scan_jobs(sj, infos)
    sj["scan"] = dev_bytes.data_ptr() + np.array(scan_at)
    sj["segs"] = dev_bytes.data_ptr() + np.array(seg_at)
    sj["coef"] = coef.data_ptr() + 2 * (GUARD + offs[:-1])
    sj["ws_off"], sj["ws_bytes"], sj["scan_bytes"], sj["nseg"] = ws_off[:-1], ws, scan_bytes, nseg
    jd = _t(sj.view(np.uint8))
    _jpeglib.check(_jpeglib.lib().x3djpeg_entropy_decode_batch(jd.data_ptr(), n, sub_bits, workspace.data_ptr(),
                                                               workspace.numel(), status.data_ptr(), stream()))
    torch.cuda.synchronize()
    assert bool((coef[:GUARD] == 0x5A5A).all()) and bool((coef[GUARD + total:] == 0x5A5A).all()), "guard overwritten"
    rounds = [int(workspace[int(o):int(o) + 4].view(torch.int32)[0]) for o in ws_off[:-1]]
    return status.cpu().numpy(), [coef[GUARD + offs[i]:GUARD + offs[i + 1]] for i in range(n)], rounds


# --------------------------------------------------------------------------- coefficients
@pytest.mark.parametrize("sub_bits", jc.SUB_BITS)
def test_coefficients_equal_the_host_decoder_case_by_case(sub_bits):
    for name in NAMES:
        rc, info, want = _host_coef(GOOD[name])
        assert rc == 0
        status, (got,), (rounds,) = _device_coefs([GOOD[name]], sub_bits)
        assert status[0] == 0 and torch.equal(got, _t(want)), (name, sub_bits)
        nsub = sum(max(1, -(-8 * int(s[1]) // sub_bits)) for s in _jpeglib.scan_prepare(GOOD[name], info)[2])
        assert 1 <= rounds <= nsub, (name, sub_bits, rounds, nsub)


@pytest.mark.parametrize("sub_bits", jc.SUB_BITS)
def test_coefficients_equal_the_host_decoder_in_one_mixed_batch(sub_bits):
    status, got, _ = _device_coefs([GOOD[n] for n in NAMES], sub_bits)
    assert not status.any()
    for name, g in zip(NAMES, got):
        assert torch.equal(g, _t(_host_coef(GOOD[name])[2])), (name, sub_bits)


# --------------------------------------------------------------------------- pixels
@pytest.fixture(scope="module")
def dec():
    return jpegops.JpegDecoder(DEV, threads=4, entropy="device")


@pytest.fixture(scope="module")
def host_dec():
    return jpegops.JpegDecoder(DEV, threads=4)


def test_entropy_and_sub_bits_are_checked():
    assert jpegops.JpegDecoder(DEV).entropy == "host"
    d = jpegops.JpegDecoder(DEV, entropy="device", sub_bits=256, check=False)
    assert (d.entropy, d.sub_bits, d.check) == ("device", 256, False)
    assert jpegops.JpegDecoder(DEV, entropy="device").sub_bits == _jpeglib.SUB_BITS_DEFAULT
    for kw in (dict(entropy="gpu"), dict(entropy="device", sub_bits=48), dict(entropy="device", sub_bits=0)):
        with pytest.raises(ValueError):
            jpegops.JpegDecoder(DEV, **kw)


def test_decode_equals_pillow_on_the_goldens(dec):
    names = [k for k, v in OLD.items() if v[1] is not None]
    outs = dec.decode([OLD[k][0] for k in names])
    for k, o in zip(names, outs):
        assert o.dtype == torch.uint8 and torch.equal(o, _t(OLD[k][1])), k
    for k in ("c420_17x9", "c420_64x48_restart", "grey_30x44"):              # and alone
        assert torch.equal(dec.decode([OLD[k][0]])[0], _t(OLD[k][1])), k
    assert not dec.last_status.any()


def test_decode_of_the_new_cases_equals_the_host_path_and_pillow(dec, host_dec):
    names = list(NEW)
    outs = dec.decode([NEW[k][0] for k in names])
    want = host_dec.decode([NEW[k][0] for k in names])
    for k, o, w in zip(names, outs, want):
        assert torch.equal(o, w), k
        if NEW[k][1] is not None:
            assert torch.equal(o, _t(NEW[k][1])), k
    assert dec.last_bytes_copied * 4 < host_dec.last_bytes_copied            # scan bytes, not coefficients


@pytest.mark.parametrize("name", ["c420_37x53_q75", "c420_40x24_blocks1"])
def test_decode_into_a_strided_slot_leaves_the_guards_alone(dec, name):
    data, rgb = (OLD if name in OLD else NEW)[name]
    H, W, _ = rgb.shape
    pitch = 3 * W + 16
    raw = torch.full((4, H, pitch), 0xA5, dtype=torch.uint8, device=DEV)   # guard frame, two slots, guard frame
    dst = raw.as_strided((2, H, W, 3), (H * pitch, pitch, 3, 1), H * pitch)
    assert dec.decode_into([data, data], dst) is dst
    want = _t(rgb)
    assert torch.equal(dst[0], want) and torch.equal(dst[1], want)
    assert bool((raw[0] == 0xA5).all()) and bool((raw[3] == 0xA5).all())
    assert bool((raw[1:3, :, 3 * W:] == 0xA5).all())


# --------------------------------------------------------------------------- damaged streams
def _corrupt_streams(count=5):
    """reject_truncated and the first `count` damaged streams of jc.damaged that parse and prepare but that the host
    decoder refuses: the streams of the sanitised CPU run, nothing else."""
    out = [("reject_truncated", OLD["reject_truncated"][0])]
    for label, data in jc.damaged(GOOD):
        if len(out) > count:
            break
        rc, info, _ = _jpeglib.parse(data)
        if rc:
            continue
        if _host_coef(data)[0] == _jpeglib.ECORRUPT and _jpeglib.scan_prepare(data, info)[0] == 0:
            out.append((label, data))
    assert len(out) == count + 1
    return out


def test_a_damaged_frame_fails_alone():
    bad = _corrupt_streams()
    a, b = GOOD["c420_37x53_q75"], GOOD["c420_64x48_restart"]
    datas = [a] + [d for _, d in bad[:3]] + [b] + [d for _, d in bad[3:]] + [a]
    good_at = (0, 4, len(datas) - 1)
    for sub_bits in (128, 1024):
        status, got, _ = _device_coefs(datas, sub_bits)                      # checks the guards
        for i, d in enumerate(datas):
            if i in good_at:
                assert status[i] == 0 and torch.equal(got[i], _t(_host_coef(d)[2])), (i, sub_bits)
            else:
                assert status[i] == _jpeglib.ECORRUPT, (i, sub_bits, status)


def test_decode_raises_naming_the_frame_and_check_false_leaves_the_status(dec, host_dec):
    (_, bad), (_, bad2) = _corrupt_streams()[:2]
    good = OLD["c420_37x53_q75"]
    with pytest.raises(X3DHipError, match=r"frame 1 of the batch.*corrupt"):
        dec.decode([good[0], bad, good[0]])
    with pytest.raises(X3DHipError, match=r"frame 2 of the batch.*corrupt"):
        dec.decode([good[0], good[0], bad2])
    quiet = jpegops.JpegDecoder(DEV, threads=2, entropy="device", check=False)
    outs = quiet.decode([good[0], bad, good[0]])
    assert quiet.last_status.cpu().tolist()[0::2] == [0, 0] and int(quiet.last_status[1]) == _jpeglib.ECORRUPT
    assert torch.equal(outs[0], _t(good[1])) and torch.equal(outs[2], _t(good[1]))
    assert torch.equal(dec.decode([good[0]])[0], _t(good[1]))                # the decoder is still usable
    # a file the headers already refuse never reaches the device
    with pytest.raises(X3DHipError, match=r"frame 1 of the batch.*progressive"):
        dec.decode([good[0], OLD["reject_progressive"][0]])


# --------------------------------------------------------------------------- graph capture
def test_a_captured_batch_replays_to_the_eager_result(dec):
    names = ["c420_120x90_q50", "c420_64x48_restart", "grey_30x44", "c420_40x24_blocks1"]
    datas = [GOOD[n] for n in names]
    eager = dec.decode(datas)
    outs = [torch.zeros_like(e) for e in eager]
    batch = dec._stage_device(datas, lambda infos: [(o.data_ptr(), 3 * o.shape[1]) for o in outs])
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        with torch.cuda.graph(graph, stream=s):
            dec.launch_device(batch)
    torch.cuda.current_stream().wait_stream(s)
    for _ in range(2):
        for o in outs:
            o.fill_(0xA5)
        batch["coef"].fill_(0x5A5A)
        batch["status"].fill_(77)
        graph.replay()
        torch.cuda.synchronize()
        assert not batch["status"].any()
        for n, o, e in zip(names, outs, eager):
            assert torch.equal(o, e), n


# --------------------------------------------------------------------------- datasets
def _folder(tmp_path):
    path = str(tmp_path / "video")
    os.makedirs(path)
    for t in range(12):
        with open(os.path.join(path, frames.FRAME_NAME.format(t + 1)), "wb") as f:
            f.write(OLD["vid_%02d" % t][0])
    return path


def test_folder_kinetics_and_decode_folder_read_the_same_either_way(tmp_path):
    path = _folder(tmp_path)
    kw = dict(sample_duration=8, gamma_tau=2, crop_size=32, x3d_version='M', device=DEV, threads=2)
    a = frames.FolderKinetics([path, path], [3, 5], rng=random.Random(99), entropy="device", **kw)
    b = frames.FolderKinetics([path, path], [3, 5], rng=random.Random(99), **kw)
    assert a.decoder.entropy == "device" and b.decoder.entropy == "host"
    va, ya = a.val_batch([0, 1], crops=3, sample_duration=10)
    vb, yb = b.val_batch([0, 1], crops=3, sample_duration=10)
    assert tuple(va.shape) == (2, 3, 3, 5, 32, 32) and torch.equal(va, vb) and torch.equal(ya, yb)
    ca, cb = a.batch([0, 1, 1], 1, 3), b.batch([0, 1, 1], 1, 3)
    assert torch.equal(ca[0], cb[0]) and torch.equal(ca[1], cb[1])
    whole = _t(np.stack([OLD["vid_%02d" % t][1] for t in range(12)]))
    assert torch.equal(frames.decode_folder(path, DEV, threads=2, chunk=5, entropy="device"), whole)
    assert torch.equal(frames.decode_folder(frames.FrameFolder(path, entropy="device"), DEV, threads=2), whole)
