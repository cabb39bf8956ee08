"""Device-resident APMeter, checks that need no GPU: the fp64 restatement (tests/apmeter_ref.py) against the reference's
golden values and on ties / -0.0 / NaN, the evaluation library's C ABI (include/x3deval.h <-> x3dhip/_evallib.py <->
exports), and the host-side argument checks of APMeter.add / add_logits."""
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from tests import apmeter_ref
from x3dhip import _evallib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "apmeter_cases.npz")


def golden_cases():
    """{name: (adds, ap)}: adds is a list of dicts with the case's inputs (scores / targets / weights, or logits of the
    cls and loc cases)."""
    z = np.load(GOLDEN)
    cases = {}
    for name in [str(c) for c in z["cases"]]:
        adds = []
        for i in range(int(z["%s__nadds" % name])):
            a = {}
            for f in ("scores", "targets", "weights", "logits", "labels", "masks"):
                key = "%s__add%d_%s" % (name, i, f)
                if key in z:
                    a[f] = z[key]
            adds.append(a)
        extra = {"n_crops": int(z["%s__n_crops" % name])} if "%s__n_crops" % name in z else {}
        cases[name] = (adds, z["%s__ap" % name], extra)
    return cases


def restated_rows(name, adds, extra):
    """The rows the reference added for a golden case, recomputed in numpy (fp32 arithmetic of the scripts)."""
    if name == "cls_crops":
        n = extra["n_crops"]
        s = [1.0 / (1.0 + np.exp(-a["logits"].astype(np.float64))) for a in adds]
        s = [x.reshape(-1, n, x.shape[1]).max(1) for x in s]
        return np.concatenate(s, 0), np.concatenate([a["targets"] for a in adds], 0), None
    if name == "loc_frames":
        S, Y = [], []
        for a in adds:
            TL = a["labels"].shape[2]
            p = 1.0 / (1.0 + np.exp(-apmeter_ref.interp_linear(a["logits"], TL).astype(np.float64)))
            p = p * a["masks"][:, None, :]
            valid = np.clip(a["masks"].sum(1).astype(np.int64), 0, TL)
            for b in range(p.shape[0]):
                S.append(p[b, :, :valid[b]].T)
                Y.append(a["labels"][b, :, :valid[b]].T)
        return np.concatenate(S, 0), np.concatenate(Y, 0), None
    w = np.concatenate([a["weights"] for a in adds]) if "weights" in adds[0] else None
    return np.concatenate([a["scores"] for a in adds], 0), np.concatenate([a["targets"] for a in adds], 0), w


@pytest.mark.parametrize("name", [str(c) for c in np.load(GOLDEN)["cases"]])
def test_restatement_matches_reference_golden(name):
    adds, ap, extra = golden_cases()[name]
    s, y, w = restated_rows(name, adds, extra)
    got = apmeter_ref.average_precision(s, y, w)
    assert got.shape == ap.shape
    np.testing.assert_allclose(got, ap.astype(np.float64), rtol=0, atol=1e-6)


def test_golden_has_a_class_without_positives():
    adds, ap, _ = golden_cases()["nopos"]
    assert all(int(a["targets"][:, 3].sum()) == 0 for a in adds) and ap[3] == 0.0


def test_restatement_ties_zero_and_nan():
    # stable: tied scores keep insertion order
    s = np.array([0.5, 0.5, 0.5, 0.9], np.float32)
    assert list(apmeter_ref.descending_order(s)) == [3, 0, 1, 2]
    # the positive first among ties -> precision 1; last -> 1/3 at rank 3 (after 0.9, which is negative: 1/4)
    assert apmeter_ref.average_precision(s[:3, None], np.array([[1], [0], [0]]))[0] == 1.0
    assert apmeter_ref.average_precision(s[:3, None], np.array([[0], [0], [1]]))[0] == pytest.approx(1 / 3)
    # -0.0 ties +0.0 (insertion order), NaN above +inf
    s = np.array([-0.0, 0.0, np.inf, np.nan, -1.0, np.nan], np.float32)
    assert list(apmeter_ref.descending_order(s)) == [3, 5, 2, 0, 1, 4]
    s = np.array([0.0, -0.0], np.float32)
    assert list(apmeter_ref.descending_order(s)) == [0, 1]
    ap = apmeter_ref.average_precision(np.array([[np.nan], [np.inf], [1.0]], np.float32), np.array([[0], [1], [1]]))
    assert ap[0] == pytest.approx((1 / 2 + 2 / 3) / 2)
    # weights: rank and tp are weighted sums
    ap = apmeter_ref.average_precision(np.array([[0.9], [0.8], [0.7]]), np.array([[0], [1], [1]]), np.array([2.0, 1.0, 1.0]))
    assert ap[0] == pytest.approx((1 / 3 + 2 / 4) / 2)


def _header_functions():
    src = open(os.path.join(ROOT, "include", "x3deval.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(x3deval_[a-z0-9_]+)\s*\(", src)))


def test_eval_header_and_ctypes_table_agree():
    assert _header_functions() == sorted(_evallib.SIGNATURES.keys())


def test_eval_library_loads_and_exports_every_symbol():
    if not os.path.exists(_evallib.LIB_PATH):
        import __graft_entry__ as ge
        ge.build()
    h = _evallib.lib()
    assert h.x3deval_abi_version() == _evallib.ABI_VERSION
    out = subprocess.run(["nm", "-D", "--defined-only", _evallib.LIB_PATH], capture_output=True, text=True).stdout
    exported = set(re.findall(r"\bT (x3deval_[a-z0-9_]+)", out))
    assert set(_header_functions()) <= exported
    # host-only workspace query: 16 bytes per row (rounded to 64 rows) per class, classes batched under a 2 GiB cap
    assert h.x3deval_ap_workspace_bytes(157, 1850) == 157 * 16 * 1856
    assert h.x3deval_ap_workspace_bytes(157, 1 << 20) == 128 * 16 * (1 << 20)
    assert h.x3deval_ap_workspace_bytes(0, 10) == 0 and h.x3deval_ap_workspace_bytes(3, 0) == 0
    assert h.x3deval_last_error() is not None


def test_eval_missing_library_fails_loudly(monkeypatch, tmp_path):
    monkeypatch.setattr(_evallib, "_lib", None)
    monkeypatch.setattr(_evallib, "LIB_PATH", str(tmp_path / "nope.so"))
    with pytest.raises(_evallib.X3DHipError):
        _evallib.lib()


def _fresh():
    from apmeter import APMeter
    return APMeter()


def test_add_host_checks_raise_before_any_gpu_work(monkeypatch):
    from x3dhip import evalops
    launched = []
    for name in ("ap_append", "ap_append_crops", "ap_append_frames", "ap_state"):
        monkeypatch.setattr(evalops, name, lambda *a, _n=name, **k: launched.append(_n))
    m = _fresh()
    y = np.zeros((4, 3), np.int64)
    with pytest.raises(AssertionError):
        m.add(np.zeros((4, 3, 2), np.float32), y)                       # 3-D output
    with pytest.raises(AssertionError):
        m.add(np.zeros((4, 3), np.float32), np.zeros((4, 3, 1)))        # 3-D target
    with pytest.raises(AssertionError):
        m.add(np.zeros((4, 3), np.float32), np.full((4, 3), 2))         # non-binary target
    with pytest.raises(AssertionError):
        m.add(np.zeros((4, 3), np.float32), y, np.array([1.0, -1.0, 1.0, 1.0], np.float32))   # negative weight
    with pytest.raises(AssertionError):
        m.add(np.zeros((4, 3), np.float32), y, np.ones(5, np.float32))                       # wrong weight length
    with pytest.raises(AssertionError):
        m.add(np.zeros((4, 3), np.float32), np.zeros((4, 2), np.int64))                      # shape mismatch
    with pytest.raises(TypeError):
        m.add(np.zeros((4, 3), np.complex64), y)                                             # dtype
    with pytest.raises(TypeError):
        m.add([[0.5]], [[1]])                                                                # not an array
    with pytest.raises(TypeError):
        m.add_logits(torch.zeros(4, 3), y)                                                   # logits on the host
    assert launched == []
    assert m.value() == 0                                                                    # still empty


def test_add_logits_host_checks_raise_before_any_gpu_work(monkeypatch):
    """add_logits validates the shapes and dtypes of device logits before launching; with no GPU here the checks run on
    a stand-in device tensor (is_cuda patched), and no kernel wrapper may be reached."""
    from x3dhip import evalops
    import apmeter
    launched = []
    for name in ("ap_append", "ap_append_crops", "ap_append_frames", "ap_state"):
        monkeypatch.setattr(evalops, name, lambda *a, _n=name, **k: launched.append(_n))
    monkeypatch.setattr(apmeter, "_is_device", lambda x: isinstance(x, torch.Tensor))
    m = _fresh()
    y = torch.zeros(2, 5)
    with pytest.raises(ValueError):
        m.add_logits(torch.zeros(6, 5, 2), y, n_crops=3)                 # [b*n, K, 2]
    with pytest.raises(ValueError):
        m.add_logits(torch.zeros(6, 5, dtype=torch.float64), y, n_crops=3)
    with pytest.raises(ValueError):
        m.add_logits(torch.zeros(7, 5), y, n_crops=3)                    # not a multiple of n_crops
    with pytest.raises(ValueError):
        m.add_logits(torch.zeros(6, 5), torch.zeros(3, 5), n_crops=3)    # target rows != b
    with pytest.raises(ValueError):
        m.add_logits(torch.zeros(6, 5), y, n_crops=0)
    with pytest.raises(ValueError):
        m.add_frames(torch.zeros(2, 5, 4), torch.zeros(2, 5, 6), torch.zeros(2, 7))   # masks [B, TL] mismatch
    with pytest.raises(ValueError):
        m.add_frames(torch.zeros(2, 5), torch.zeros(2, 5, 6), torch.zeros(2, 6))      # logits not [B, K, T]
    assert launched == []
