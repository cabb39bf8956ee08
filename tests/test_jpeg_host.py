"""JPEG decoder, checks that need no GPU: tests/jpeg_ref.py (the numpy restatement) pinned to Pillow bit for bit on a sweep
of sizes, subsamplings and encoder settings and on the committed goldens (tests/golden/jpeg_cases.npz), the value ranges
that keep the int32 kernels on safe ground, the C ABI of libx3djpeg.so (include/x3djpeg.h <-> x3dhip/_jpeglib.py <->
exports), the library's host stage (parse, Huffman decoding) against the restatement, its behaviour on truncated and
damaged files, and the folder / annotation logic of frames.py."""
import io
import os
import re
import subprocess

import numpy as np
import pytest

import frames
from tests import jpeg_ref as jr
from x3dhip import _jpeglib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = jr.load_cases()
GOOD = {k: v for k, v in CASES.items() if v[1] is not None}
REJECTS = {k: v for k, v in CASES.items() if v[1] is None}


# --------------------------------------------------------------------------- restatement == Pillow
def _encode(arr, mode="RGB", **kw):
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(arr, mode).save(buf, "JPEG", **kw)
    return buf.getvalue()


def _pillow(data):
    from PIL import Image
    return np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))


def test_restatement_equals_pillow_on_the_size_sweep():
    pytest.importorskip("PIL.Image")
    sizes = list(range(1, 20)) + [31, 32, 33]
    rng = np.random.default_rng(7)
    n = 0
    for sub in (0, 1, 2):
        for h in sizes:
            for w in sizes:
                data = _encode(rng.integers(0, 256, (h, w, 3), dtype=np.uint8), quality=92, subsampling=sub)
                assert np.array_equal(jr.decode(data), _pillow(data)), (sub, h, w)
                n += 1
    assert n == 1452


def test_restatement_equals_pillow_on_qualities_and_encoder_options():
    pytest.importorskip("PIL.Image")
    rng = np.random.default_rng(8)
    y, x = np.mgrid[0:40, 0:56]
    smooth = np.stack([x * 4, y * 6, (x + y) * 2], axis=-1).astype(np.uint8)
    noisy = rng.integers(0, 256, (40, 56, 3), dtype=np.uint8)
    for img in (smooth, noisy):
        for q in (1, 5, 30, 50, 60, 75, 85, 90, 95, 100):
            for sub in (0, 1, 2):
                data = _encode(img, quality=q, subsampling=sub)
                assert np.array_equal(jr.decode(data), _pillow(data)), (q, sub)
        for kw in (dict(optimize=True), dict(restart_marker_blocks=3), dict(restart_marker_rows=1)):
            data = _encode(img, quality=80, subsampling=2, **kw)
            assert np.array_equal(jr.decode(data), _pillow(data)), kw
        data = _encode(img[..., 0], mode="L", quality=85)
        assert np.array_equal(jr.decode(data), _pillow(data))


# --------------------------------------------------------------------------- goldens
def test_fixture_holds_the_cases_it_is_meant_to():
    info = {k: jr.parse(v[0]) for k, v in GOOD.items()}

    def shape(k):
        i = info[k]
        return (i["width"], i["height"], len(i["comps"]), i["hmax"], i["vmax"])

    assert shape("c444_8x8") == (8, 8, 3, 1, 1)
    assert shape("c420_17x9") == (17, 9, 3, 2, 2) and shape("c420_9x17") == (9, 17, 3, 2, 2)
    assert [(info[k]["comps"][1]["cw"], info[k]["comps"][1]["ch"]) for k in ("c420_17x9", "c420_9x17")] == [(9, 5), (5, 9)]
    for k in ("c422_3x4", "c422_4x3", "c420_3x4", "c420_4x3"):
        assert info[k]["comps"][1]["cw"] <= 2 and info[k]["hmax"] == 2
    assert info["c420_5x6"]["comps"][1]["cw"] == 3
    assert shape("c422_33x70_q60") == (33, 70, 3, 2, 1) and shape("c420_37x53_q75") == (37, 53, 3, 2, 2)
    assert shape("c420_50x50_q100_noise") == (50, 50, 3, 2, 2) and all(int(q.max()) == 1 for q in
                                                                        info["c420_50x50_q100_noise"]["qt"].values())
    assert max(int(q.max()) for q in info["c420_40x56_q1"]["qt"].values()) == 255
    assert info["c420_64x48_restart"]["restart_interval"] > 0
    # optimize=True: Huffman tables that are not the standard ones of the other files
    assert info["c420_40x56_optimize"]["huff"] != info["c420_37x53_q75"]["huff"]
    assert info["c420_37x53_q75"]["huff"] == info["c420_120x90_q50"]["huff"]
    assert shape("grey_30x44") == (30, 44, 1, 1, 1) and shape("c420_120x90_q50") == (120, 90, 3, 2, 2)
    assert all(shape("vid_%02d" % t) == (64, 48, 3, 2, 2) for t in range(12))
    assert sorted(REJECTS) == ["reject_cmyk", "reject_progressive", "reject_truncated"]
    # both clamps of the colour conversion and of the IDCT are reached by some golden
    assert any(v[1].min() == 0 and v[1].max() == 255 for v in GOOD.values())
    assert os.path.getsize(os.path.join(jr.GOLDEN, "jpeg_cases.npz")) < 300 * 1024


def test_restatement_equals_every_golden_and_stays_inside_int16_and_int32():
    for name, (data, rgb) in GOOD.items():
        track = {}
        got = jr.decode(data, track)
        assert got.dtype == rgb.dtype and np.array_equal(got, rgb), name
        assert track["dequant"] < 2 ** 15, (name, track)
        assert track["idct"] < 2 ** 31, (name, track)


def test_restatement_rejects_the_rejects():
    with pytest.raises(jr.Unsupported):
        jr.decode(REJECTS["reject_progressive"][0])
    with pytest.raises(jr.Unsupported):
        jr.decode(REJECTS["reject_cmyk"][0])
    with pytest.raises(jr.Corrupt):
        jr.decode(REJECTS["reject_truncated"][0])


def test_constants_of_the_issue():
    assert [jr._fix(x) for x in (0.298631336, 0.390180644, 0.541196100, 0.765366865, 0.899976223, 1.175875602, 1.501321110,
                                 1.847759065, 1.961570560, 2.053119869, 2.562915447, 3.072711026)] == \
        [2446, 3196, 4433, 6270, 7373, 9633, 12299, 15137, 16069, 16819, 20995, 25172]
    assert [jr._g(x) for x in (1.402, 1.772, 0.34414, 0.71414)] == [91881, 116130, 22554, 46802]
    src = open(os.path.join(ROOT, "x3d-multigrid_amd", "csrc_jpeg", "kernels.hip")).read()
    for name, v in (("FIX_0_298631336", 2446), ("FIX_3_072711026", 25172), ("G_1_402", 91881), ("G_0_71414", 46802)):
        assert re.search(r"\b%s = %d\b" % (name, v), src), name


# --------------------------------------------------------------------------- C ABI
def _header_functions():
    src = open(os.path.join(ROOT, "include", "x3djpeg.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(x3djpeg_[a-z0-9_]+)\s*\(", src)))


def _lib():
    if not os.path.exists(_jpeglib.LIB_PATH):
        import __graft_entry__ as ge
        ge.build()
    return _jpeglib.lib()


def test_jpeg_header_and_ctypes_table_agree():
    assert _header_functions() == sorted(_jpeglib.SIGNATURES.keys())


def test_jpeg_library_loads_and_exports_every_symbol():
    h = _lib()
    assert h.x3djpeg_abi_version() == _jpeglib.ABI_VERSION
    out = subprocess.run(["nm", "-D", "--defined-only", _jpeglib.LIB_PATH], capture_output=True, text=True).stdout
    exported = set(re.findall(r"\bT (x3djpeg_[a-z0-9_]+)", out))
    assert set(_header_functions()) == exported
    assert h.x3djpeg_info_bytes() == _jpeglib.INFO_DT.itemsize
    assert h.x3djpeg_frame_job_bytes() == _jpeglib.FRAME_JOB_DT.itemsize == 512
    assert _jpeglib.FRAME_JOB_DT.fields["qt"][1] % 16 == 0
    # argument checks happen on the host, before any launch
    assert h.x3djpeg_parse(None, 0, None) == _jpeglib.EINVAL
    assert h.x3djpeg_idct(None, 1, 1, None) == _jpeglib.EINVAL and b"argument check failed" in h.x3djpeg_last_error()
    assert h.x3djpeg_to_rgb(None, 1, 1, 1, None) == _jpeglib.EINVAL
    assert h.x3djpeg_decode_batch(None, 1, 1, 1, 1, None) == _jpeglib.EINVAL


def test_jpeg_missing_library_fails_loudly(monkeypatch, tmp_path):
    monkeypatch.setattr(_jpeglib, "_lib", None)
    monkeypatch.setattr(_jpeglib, "LIB_PATH", str(tmp_path / "nope.so"))
    with pytest.raises(_jpeglib.X3DHipError):
        _jpeglib.lib()


def test_stamp_covers_the_jpeg_library_and_leaves_the_training_stamp_alone():
    from tools import stamp
    a = stamp.csrc_jpeg_sha16()
    assert re.fullmatch(r"[0-9a-f]{16}", a)
    assert len({a, stamp.csrc_sha16(), stamp.csrc_eval_sha16(), stamp.csrc_data_sha16()}) == 4


# --------------------------------------------------------------------------- the library's host stage
def _host_decode(data, guard=32):
    """(rc, info, coefficients or None, message) with `guard` int16 canaries (64 bytes) on either side of the buffer."""
    _lib()
    rc, info, msg = _jpeglib.parse(data)
    if rc:
        return rc, info, None, msg
    n = int(info["coef_count"][0])
    buf = np.full(n + 2 * guard, 0x5A5A, dtype=np.int16)
    rc, msg = _jpeglib.entropy_decode(data, info, buf.ctypes.data + 2 * guard, 2 * n)
    assert np.all(buf[:guard] == 0x5A5A) and np.all(buf[guard + n:] == 0x5A5A), "canary overwritten"
    return rc, info, buf[guard:guard + n], msg


def test_host_stage_headers_and_coefficients_equal_the_restatement():
    for name, (data, _) in GOOD.items():
        rc, info, coef, msg = _host_decode(data)
        assert rc == 0, (name, msg)
        ref = jr.parse(data)
        i = info[0]
        assert (i["width"], i["height"], i["ncomp"], i["hmax"], i["vmax"]) == \
            (ref["width"], ref["height"], len(ref["comps"]), ref["hmax"], ref["vmax"]), name
        assert i["restart_interval"] == ref["restart_interval"] and i["scan_off"] == ref["scan_off"]
        want = jr.entropy_decode(data, ref)
        for c, (comp, w) in enumerate(zip(ref["comps"], want)):
            assert (i["blocks_w"][c], i["blocks_h"][c], i["cw"][c], i["ch"][c]) == \
                (comp["blocks_w"], comp["blocks_h"], comp["cw"], comp["ch"]), name
            assert np.array_equal(i["qt"][comp["tq"]], ref["qt"][comp["tq"]]), name
            off = int(i["coef_off"][c])
            assert off == 64 * int(i["block_start"][c])
            assert np.array_equal(coef[off:off + w.size], w.ravel()), (name, c)
        assert int(i["coef_count"]) == sum(w.size for w in want) == 64 * int(i["nblocks"])


def test_host_stage_rejects_name_the_feature():
    rc, _, _, msg = _host_decode(REJECTS["reject_progressive"][0])
    assert rc == _jpeglib.EUNSUPPORTED and "progressive" in msg
    rc, _, _, msg = _host_decode(REJECTS["reject_cmyk"][0])
    assert rc == _jpeglib.EUNSUPPORTED and "4 components" in msg
    rc, _, _, msg = _host_decode(REJECTS["reject_truncated"][0])
    assert rc == _jpeglib.ECORRUPT and "scan data ends" in msg


def _patched(data, marker, offset, value):
    """data with the byte at `offset` after the first `marker` set to value."""
    i = data.index(marker) + offset
    return data[:i] + bytes([value]) + data[i + 1:]


def test_host_stage_rejects_other_unsupported_kinds_by_name():
    _lib()
    data = GOOD["c420_37x53_q75"][0]
    sof = b"\xff\xc0"
    for patch, word in (((sof, 1, 0xC9), "arithmetic"), ((sof, 1, 0xC3), "lossless"), ((sof, 4, 12), "12-bit"),
                        ((sof, 11, 0x12), "sampling factors"), ((sof, 11, 0x41), "sampling factors")):
        rc, _, msg = _jpeglib.parse(_patched(data, *patch))
        assert rc == _jpeglib.EUNSUPPORTED and word in msg, (patch, rc, msg)
    # a scan that holds one of the three components: a multi-scan file
    i = data.index(b"\xff\xda")
    one = data[:i] + b"\xff\xda\x00\x08\x01\x01\x00\x00\x3f\x00" + data[i + 14:]
    rc, _, msg = _jpeglib.parse(one)
    assert rc == _jpeglib.EUNSUPPORTED and "multi-scan" in msg
    # Adobe APP14 with transform 0 (RGB) in front of a 3-component frame
    adobe = data[:2] + b"\xff\xee\x00\x0eAdobe\x00\x64\x00\x00\x00\x00\x00" + data[2:]
    rc, _, msg = _jpeglib.parse(adobe)
    assert rc == _jpeglib.EUNSUPPORTED and "Adobe" in msg
    rc, _, msg = _jpeglib.parse(adobe[:17] + b"\x01" + adobe[18:])
    assert rc == 0, msg
    # a 16-bit quantisation table is read like an 8-bit one
    j = data.index(b"\xff\xdb")
    L = (data[j + 2] << 8) | data[j + 3]
    seg = data[j + 4:j + 2 + L]
    assert L == 67 and seg[0] >> 4 == 0
    wide = bytes([0x10 | seg[0]]) + b"".join(bytes([0, v]) for v in seg[1:])
    data16 = data[:j] + b"\xff\xdb" + (len(wide) + 2).to_bytes(2, "big") + wide + data[j + 2 + L:]
    rc, info, coef, msg = _host_decode(data16)
    rc0, info0, coef0, _ = _host_decode(data)
    assert rc == 0 and np.array_equal(info["qt"], info0["qt"]) and np.array_equal(coef, coef0), msg


def test_truncations_and_byte_flips_never_leave_the_buffers():
    data = GOOD["c420_17x9"][0]
    allowed = {_jpeglib.OK, _jpeglib.ECORRUPT, _jpeglib.EUNSUPPORTED}
    seen = set()
    for n in range(len(data) + 1):
        rc = _host_decode(data[:n])[0]
        assert rc in allowed, (n, rc)
        seen.add(rc)
    assert _host_decode(data[:len(data) // 2])[0] == _jpeglib.ECORRUPT
    rng = np.random.default_rng(2024)
    for name in ("c420_17x9", "c420_64x48_restart"):
        data = GOOD[name][0]
        for _ in range(1000):
            b = bytearray(data)
            for _ in range(int(rng.integers(1, 4))):
                b[int(rng.integers(0, len(b)))] = int(rng.integers(0, 256))
            rc = _host_decode(bytes(b))[0]
            assert rc in allowed, rc
            seen.add(rc)
    assert {_jpeglib.OK, _jpeglib.ECORRUPT} <= seen


# --------------------------------------------------------------------------- frame folders and the annotation listing
def _write_folder(path, n, data):
    os.makedirs(path)
    for i in range(1, n + 1):
        with open(os.path.join(path, frames.FRAME_NAME.format(i)), "wb") as f:
            f.write(data[(i - 1) % len(data)])


def test_frame_folder_reads_what_the_listing_and_the_first_header_say(tmp_path):
    _lib()
    vid = [CASES["vid_%02d" % t][0] for t in range(12)]
    _write_folder(str(tmp_path / "v"), 12, vid)
    os.remove(str(tmp_path / "v" / "frame_00010.jpg"))                  # a gap: the video ends before it
    with open(str(tmp_path / "v" / "notes.txt"), "w") as f:
        f.write("x")
    ff = frames.FrameFolder(str(tmp_path / "v"))
    assert (ff.n_frames, ff.width, ff.height) == (9, 64, 48)
    assert ff.read([0, 8, 3]) == [vid[0], vid[8], vid[3]]
    with pytest.raises(ValueError):
        ff.read([9])
    os.makedirs(str(tmp_path / "empty"))
    with pytest.raises(ValueError):
        frames.FrameFolder(str(tmp_path / "empty"))
    _write_folder(str(tmp_path / "bad"), 1, [REJECTS["reject_progressive"][0]])
    with pytest.raises(_jpeglib.X3DHipError, match="progressive"):
        frames.FrameFolder(str(tmp_path / "bad"))


def test_annotation_listing_names_labels_and_skips(tmp_path):
    _lib()
    anno = {
        "aaa": {"subset": "train", "annotations": {"label": "riding a bike", "segment": [3.0, 13.9]}},
        "bbb": {"subset": "train", "annotations": {"label": "abseiling", "segment": [120, 130]}},        # 81 frames: skipped
        "ccc": {"subset": "train", "annotations": {"label": "zumba", "segment": [0, 10]}},               # no folder: skipped
        "ddd": {"subset": "validation", "annotations": {"label": "riding a bike"}},
    }
    labels = ["abseiling", "riding a bike", "zumba"]
    assert frames.video_names_and_labels(anno, "train") == [
        ("riding_a_bike/aaa_000003_000013", "riding a bike"), ("abseiling/bbb_000120_000130", "abseiling"),
        ("zumba/ccc_000000_000010", "zumba")]
    assert frames.video_names_and_labels(anno, "validation") == [("riding_a_bike/ddd", "riding a bike")]
    assert frames.video_names_and_labels({"t": {"subset": "testing"}}, "testing") == [("test/t", None)]
    assert frames.class_labels(labels) == {"abseiling": 0, "riding a bike": 1, "zumba": 2}
    vid = [CASES["vid_%02d" % t][0] for t in range(12)]
    root = str(tmp_path)
    _write_folder(os.path.join(root, "riding_a_bike", "aaa_000003_000013"), 82, vid)
    _write_folder(os.path.join(root, "abseiling", "bbb_000120_000130"), 81, vid)
    _write_folder(os.path.join(root, "riding_a_bike", "ddd"), 90, vid)
    got = frames.list_dataset(root, anno, frames.class_labels(labels), "train")
    assert [(os.path.relpath(f.path, root), f.n_frames, (f.width, f.height), y) for f, y in got] == \
        [(os.path.join("riding_a_bike", "aaa_000003_000013"), 82, (64, 48), 1)]
    got = frames.list_dataset(root, anno, frames.class_labels(labels), "validation")
    assert [(os.path.relpath(f.path, root), f.n_frames, y) for f, y in got] == [(os.path.join("riding_a_bike", "ddd"), 90, 1)]
