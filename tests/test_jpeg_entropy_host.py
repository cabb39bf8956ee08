"""The parallel Huffman decoder of libx3djpeg.so, checks that need no GPU: x3djpeg_scan_prepare against a plain restatement
of unstuffing and segment cutting, x3djpeg_entropy_decode_parallel_host (the kernel's code, run serially) against the host
decoder x3djpeg_entropy_decode bit for bit at three subsequence lengths, damaged streams, and the same cases once more in
a stand-alone program built with the address and undefined-behaviour sanitisers."""
import os
import re
import shutil
import struct
import subprocess

import numpy as np
import pytest

from tests import jpeg_entropy_cases as jc
from tests import jpeg_ref as jr
from x3dhip import _jpeglib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOOD = jc.good_cases()
GUARD = 32          # int16 elements on either side of a coefficient buffer


def _lib():
    if not os.path.exists(_jpeglib.LIB_PATH):
        import __graft_entry__ as ge
        ge.build()
    return _jpeglib.lib()


def _parse(data):
    _lib()
    rc, info, msg = _jpeglib.parse(data)
    return rc, info


def _host(data, info):
    n = int(info["coef_count"][0])
    buf = np.full(n + 2 * GUARD, 0x5A5A, dtype=np.int16)
    rc, _ = _jpeglib.entropy_decode(data, info, buf.ctypes.data + 2 * GUARD, 2 * n)
    assert np.all(buf[:GUARD] == 0x5A5A) and np.all(buf[GUARD + n:] == 0x5A5A)
    return rc, buf[GUARD:GUARD + n]


def _parallel(data, info, sub_bits):
    """(status or prepare's error, coefficients, rounds, subsequences); the guards checked."""
    n = int(info["coef_count"][0])
    buf = np.full(n + 2 * GUARD, 0x5A5A, dtype=np.int16)
    st, rounds, nsub, _ = _jpeglib.entropy_decode_parallel_host(data, info, buf.ctypes.data + 2 * GUARD, sub_bits)
    assert np.all(buf[:GUARD] == 0x5A5A) and np.all(buf[GUARD + n:] == 0x5A5A), "guard overwritten"
    return st, buf[GUARD:GUARD + n], rounds, nsub


def test_new_symbols_structs_and_argument_checks():
    h = _lib()
    assert _jpeglib.ABI_VERSION == 2 and h.x3djpeg_abi_version() == 2
    assert h.x3djpeg_scan_seg_bytes() == _jpeglib.SCAN_SEG_DT.itemsize == 16
    assert h.x3djpeg_scan_job_bytes() == _jpeglib.SCAN_JOB_DT.itemsize and _jpeglib.SCAN_JOB_DT.itemsize % 16 == 0
    src = open(os.path.join(ROOT, "include", "x3djpeg.h")).read()
    assert re.search(r"#define X3DJPEG_SCAN_PAD %d\b" % _jpeglib.SCAN_PAD, src)
    assert re.search(r"#define X3DJPEG_SUB_BITS_DEFAULT %d\b" % _jpeglib.SUB_BITS_DEFAULT, src)
    assert jc.SUB_BITS[-1] == _jpeglib.SUB_BITS_DEFAULT
    assert h.x3djpeg_scan_prepare(None, 0, None, None, 0, None, 0, None, None) == _jpeglib.EINVAL
    assert h.x3djpeg_entropy_decode_parallel_host(None, 1, 1024, None, 0, None, None) == _jpeglib.EINVAL
    assert h.x3djpeg_entropy_decode_batch(None, 1, 1024, None, 0, None, None) == _jpeglib.EINVAL
    assert h.x3djpeg_entropy_workspace_bytes(1000, 1, 48) == 0 and h.x3djpeg_entropy_workspace_bytes(1000, 1, 0) == 0
    assert h.x3djpeg_entropy_workspace_bytes(1000, 1, 32) % 16 == 0 and h.x3djpeg_entropy_workspace_bytes(1000, 1, 32) > 0
    # too small a scan buffer or segment table is refused, not overrun
    data = GOOD["c420_64x48_restart"]
    rc, info = _parse(data)
    scan, segs, out = np.zeros(64, np.uint8), np.zeros(64, _jpeglib.SCAN_SEG_DT), np.zeros(2, np.uint64)
    args = (data, len(data), info.ctypes.data, scan.ctypes.data)
    assert h.x3djpeg_scan_prepare(*args, 40, segs.ctypes.data, 64, out.ctypes.data, out.ctypes.data + 8) == _jpeglib.EINVAL
    assert h.x3djpeg_scan_prepare(*args, 8, segs.ctypes.data, 64, out.ctypes.data, out.ctypes.data + 8) == _jpeglib.EINVAL
    assert not scan[40:].any()
    big = np.zeros(len(data), np.uint8)
    assert h.x3djpeg_scan_prepare(data, len(data), info.ctypes.data, big.ctypes.data, big.size, segs.ctypes.data, 1,
                                  out.ctypes.data, out.ctypes.data + 8) == _jpeglib.EINVAL


def test_the_fixture_holds_the_cases_it_is_meant_to():
    cases = jc.load_entropy_cases()
    assert list(cases) == ["c420_340x256_q75", "c420_340x256_q75_rows", "c420_320x240_q5", "c422_161x99_optimize",
                           "grey_200x150", "flat_512x512", "c420_40x24_blocks1", "c444_48x40_q95_noise"]
    assert [k for k, v in cases.items() if v[1] is not None] == ["c420_40x24_blocks1", "c444_48x40_q95_noise"]
    assert os.path.getsize(os.path.join(jr.GOLDEN, "jpeg_entropy_cases.npz")) < 200 * 1024
    stats = {}
    for name, (data, _) in cases.items():
        info = jr.parse(data)
        mcus = info["mcus_x"] * info["mcus_y"]
        scan, segs = jc.unstuff(data, info["scan_off"], mcus, info["restart_interval"])
        stuffed = data[info["scan_off"]:].count(b"\xff\x00")
        stats[name] = (len(segs), sum(max(1, -(-8 * s[1] // 1024)) for s in segs), stuffed, max(s[1] for s in segs), info)
    assert stats["c420_340x256_q75"][:2] == (1, 272) and stats["c420_340x256_q75"][2] > 0       # > 256 threads
    assert stats["c420_340x256_q75_rows"][0] == 16 and stats["c420_340x256_q75_rows"][1] > 256
    assert stats["c420_320x240_q5"][3] * 8 < 24 * 1800                                          # bits per block
    assert stats["c422_161x99_optimize"][4]["huff"] != stats["c420_340x256_q75"][4]["huff"]
    assert len(stats["grey_200x150"][4]["comps"]) == 1
    assert stats["flat_512x512"][2:4] == (0, 4096)                                              # 32 bits per MCU
    assert stats["c420_40x24_blocks1"][0] == 6 and stats["c420_40x24_blocks1"][3] * 8 <= 1024
    assert stats["c444_48x40_q95_noise"][4]["hmax"] == 1 and stats["c444_48x40_q95_noise"][2] > 0


@pytest.mark.parametrize("name", list(GOOD))
def test_scan_prepare_equals_the_restatement(name):
    data = GOOD[name]
    rc, info = _parse(data)
    assert rc == 0
    i = info[0]
    want_scan, want_segs = jc.unstuff(data, int(i["scan_off"]), int(i["mcus_x"]) * int(i["mcus_y"]), int(i["restart_interval"]))
    rc, scan, segs, msg = _jpeglib.scan_prepare(data, info)
    assert rc == 0, msg
    assert scan[:-_jpeglib.SCAN_PAD].tobytes() == want_scan and not scan[-_jpeglib.SCAN_PAD:].any()
    assert [tuple(int(v) for v in s) for s in segs] == want_segs


@pytest.mark.parametrize("sub_bits", jc.SUB_BITS)
def test_parallel_host_equals_the_host_decoder(sub_bits):
    """Relaxation rounds of flat_512x512 (a strictly periodic stream of 32 bits per MCU: every subsequence boundary is an
    MCU boundary, so the guessed entry states are already exact): 1 of 1024 / 256 / 32 subsequences at sub_bits 32 / 128 /
    1024.  c420_340x256_q75, the training-sized frame: 195 of 8695, 49 of 2174, 6 of 272.  The slowest is
    c420_50x50_q100_noise with 1345 of 1412, 337 of 353, 40 of 45: the bit position resynchronises within a few codes,
    the block index within the MCU only when a wrong guess of it happens to decode into the right one."""
    seen = {}
    for name, data in GOOD.items():
        rc, info = _parse(data)
        rc, want = _host(data, info)
        assert rc == 0, name
        st, got, rounds, nsub = _parallel(data, info, sub_bits)
        assert st == 0 and np.array_equal(got, want), (name, sub_bits)
        assert 1 <= rounds <= nsub, (name, sub_bits, rounds, nsub)
        seen[name] = (rounds, nsub)
    print(sub_bits, seen)
    assert seen["flat_512x512"][0] == 1
    assert seen["c420_340x256_q75"][1] == -(-34780 * 8 // sub_bits)


def test_damaged_streams_fail_where_the_host_decoder_fails_and_stay_inside_the_buffer():
    seen = set()
    for label, data in jc.damaged(GOOD):
        rc, info = _parse(data)
        if rc:
            continue
        rc, want = _host(data, info)
        assert rc in (_jpeglib.OK, _jpeglib.ECORRUPT), label
        seen.add(rc)
        for sub_bits in (128, 1024):
            st, got, rounds, nsub = _parallel(data, info, sub_bits)
            if rc == 0:
                assert st == 0 and np.array_equal(got, want), (label, sub_bits)
            else:
                assert st == _jpeglib.ECORRUPT, (label, sub_bits, st)
            assert st != 0 or 1 <= rounds <= nsub
    assert seen == {_jpeglib.OK, _jpeglib.ECORRUPT}


def test_prepare_rejects_an_over_subscribed_table_and_a_missing_restart_marker():
    data = GOOD["c420_64x48_restart"]
    rc, info = _parse(data)
    bad = info.copy()
    bad["huff_bits"][0, int(bad["comp_td"][0, 0]), 0] = 3          # three codes of length 1
    rc, _, _, msg = _jpeglib.scan_prepare(data, bad)
    assert rc == _jpeglib.ECORRUPT and "over-subscribed" in msg
    i = data.index(b"\xff\xd1")
    rc, _, _, msg = _jpeglib.scan_prepare(data[:i + 1] + b"\xd2" + data[i + 2:], info)
    assert rc == _jpeglib.ECORRUPT and "restart marker" in msg
    # fill bytes before a marker are accepted, as the host decoder accepts them
    filled = data[:i] + b"\xff\xff" + data[i:]
    rc, scan, segs, msg = _jpeglib.scan_prepare(filled, info)
    rc0, scan0, segs0, _ = _jpeglib.scan_prepare(data, info)
    assert rc == 0 and rc0 == 0 and np.array_equal(scan, scan0) and np.array_equal(segs, segs0)
    assert _host(filled, info)[0] == 0


def test_the_same_cases_in_a_sanitised_stand_alone_program(tmp_path):
    """host.cpp, scan.cpp and entropy_core.h compiled with -fsanitize=address,undefined into a program of their own, run as
    a child process on every good case and every damaged stream; nothing sanitised is loaded into this interpreter."""
    cxx = os.environ.get("CXX") or shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no C++ compiler"
    blobs = list(GOOD.values()) + [d for _, d in jc.damaged(GOOD)]
    path = str(tmp_path / "cases.bin")
    with open(path, "wb") as f:
        f.write(struct.pack("<I", len(blobs)))
        for b in blobs:
            f.write(struct.pack("<I", len(b)))
            f.write(b)
    src = os.path.join(ROOT, "x3d-multigrid_amd", "csrc_jpeg")
    exe = str(tmp_path / "jpeg_entropy_check")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "jpeg_entropy_check.cpp"),
           os.path.join(src, "host.cpp"), os.path.join(src, "scan.cpp"), "-o", exe]
    # the sanitisers' runtimes linked into the program itself where the compiler ships them so (gcc needs to be told)
    if subprocess.run(cmd + ["-static-libasan", "-static-libubsan"], capture_output=True).returncode != 0:
        subprocess.run(cmd, check=True)
    r = subprocess.run([exe, path], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    last = r.stdout.strip().splitlines()[-1].split()
    assert last[0] == "cases" and int(last[1]) == len(blobs) and int(last[-1]) == 0, r.stdout[-500:]
    assert int(last[3]) >= len(GOOD) and int(last[5]) > 0


def test_the_entropy_option_reaches_the_datasets(monkeypatch, tmp_path):
    import frames
    import kinetics
    seen = {}
    dataset = type("D", (), dict(sample_duration=80, gamma_tau=5))()
    monkeypatch.setattr(kinetics.FolderKinetics, "from_annotation",
                        classmethod(lambda cls, *a, **kw: seen.update(fk=kw) or dataset))
    kinetics.Kinetics("R", "A", "L", "validate", entropy="device")
    assert seen["fk"]["entropy"] == "device"
    kinetics.Kinetics("R", "A", "L", "validate")
    assert "entropy" not in seen["fk"]                        # the default: FolderKinetics' own 'host'
    _lib()
    path = tmp_path / "v"
    path.mkdir()
    (path / frames.FRAME_NAME.format(1)).write_bytes(GOOD["vid_00"])
    assert frames.FrameFolder(str(path), entropy="device").entropy == "device" and frames.FrameFolder(str(path)).entropy is None
    with pytest.raises(ValueError):
        frames.FrameFolder(str(path), entropy="gpu")
