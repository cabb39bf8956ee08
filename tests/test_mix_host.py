"""libx3dmix on the host: the twins x3dmix_clips_host and x3dmix_targets_host (the code of the kernels through mix_core.h)
against the numpy restatement tests/mix_ref.py byte for byte on hand-built plans; mixup and the targets against fp64 within
counted roundings; x3dmix_soft_ce_host against F.cross_entropy on probabilities in fp64; the BatchMixer's plans; the ABI; the
refusals; the same lists in a sanitised stand-alone program.  No GPU."""
import inspect
import os
import re
import subprocess

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import mix_cases as mc
from tests import mix_program, mix_ref
from x3dhip import _mixlib, mixing, mixops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
U = 2.0 ** -24


def _lib():
    if not os.path.exists(_mixlib.LIB_PATH):
        import __graft_entry__ as ge
        ge.build()
    return _mixlib.lib()


def _bytes_equal(a, b):
    return np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


# -- ABI --------------------------------------------------------------------------------------------------------------------
def test_mix_header_ctypes_table_and_exports_agree():
    h = _lib()
    src = open(os.path.join(ROOT, "include", "x3dmix.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    nm = subprocess.run(["nm", "-D", "--defined-only", _mixlib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exports = set(re.findall(r" T (x3dmix_[a-z0-9_]+)\n", nm))
    declared = set(re.findall(r"\b(x3dmix_[a-z0-9_]+)\s*\(", code))
    assert declared == exports == set(_mixlib.SIGNATURES)
    for name, (_, args) in _mixlib.SIGNATURES.items():
        decl = re.search(r"\b%s\s*\(([^)]*)\)" % name, code).group(1).strip()
        count = 0 if decl == "void" else len(decl.split(","))
        assert count == len(args), name
    for name in ("x3dmix_clips", "x3dmix_targets", "x3dmix_soft_ce"):       # a twin: the same arguments minus the stream
        assert _mixlib.SIGNATURES[name + "_host"][1] == _mixlib.SIGNATURES[name][1][:-1]
    assert h.x3dmix_abi_version() == 1 == _mixlib.ABI_VERSION
    assert int(re.search(r"#define X3DMIX_ABI_VERSION (\d+)", src).group(1)) == 1
    assert h.x3dmix_sample_bytes() == 32 == _mixlib.SAMPLE_DT.itemsize == _mixlib.SAMPLE_BYTES
    assert [_mixlib.SAMPLE_DT.fields[k][1] for k in ("partner", "lam", "y0", "y1", "x0", "x1", "pad")] == [0, 4, 8, 12, 16, 20, 24]


def test_stamp_has_an_identity_for_the_mixing_sources():
    from tools import stamp
    a = stamp.csrc_mix_sha16()
    assert re.fullmatch(r"[0-9a-f]{16}", a) and a != stamp.csrc_step_sha16() and a != stamp.csrc_sha16()


# -- the clips ----------------------------------------------------------------------------------------------------------------
CLIP_CASES = mc.clip_cases()


def test_clip_cases_reach_every_branch():
    """The coverage is built by hand, and counted here: every mode, every shape, the plans the rule is subtle on."""
    _lib()
    modes = set()
    for _, x, plan in CLIP_CASES:
        B, _, H, W = x.shape
        modes |= {mix_ref.resolve(plan[b], b, B, H, W)[1] for b in range(B)}
    assert modes == {"copy", "mixup", "cutmix"}
    assert {tuple(x.shape) for _, x, _ in CLIP_CASES} == set(mc.CLIP_SHAPES)
    assert (2 * 3 * 5 * 7 // 2) % 4 != 0 and (6 * 79 * 79) % 4 != 0 and 158 % 4 != 0


@pytest.mark.parametrize("name,x,plan", CLIP_CASES, ids=[c[0] for c in CLIP_CASES])
def test_clips_host_equals_the_restatement_byte_for_byte(name, x, plan):
    _lib()
    got = mixops.mix_clips_host(x, plan)
    assert _bytes_equal(got, mix_ref.mix_clips(x, plan))


def test_clips_host_writes_nothing_outside_its_output_and_leaves_the_source_alone():
    _lib()
    x = mc.normals((3, 6, 79, 79), 11)
    plan = mc.plans(3, 79, 79)["modes_by_sample"]
    n = x.size
    buf = np.full(n + 64, F32(7.5))
    out = buf[32:32 + n].reshape(x.shape)
    keep = x.copy()
    mixops.mix_clips_host(x, plan, out=out)
    assert _bytes_equal(x, keep) and np.all(buf[:32] == F32(7.5)) and np.all(buf[32 + n:] == F32(7.5))
    assert _bytes_equal(out, mix_ref.mix_clips(x, plan))


NAN_CASES = mc.nan_cases()


@pytest.mark.parametrize("name,x,plan,expected", NAN_CASES, ids=[c[0] for c in NAN_CASES])
def test_cutmix_is_a_select_and_lam_one_is_a_bit_copy(name, x, plan, expected):
    """The partner NaN outside the box and the sample NaN inside it: the output is the expected bits with no NaN in the
    CutMix sample; lam == 1 with a NaN partner is a copy."""
    _lib()
    got = mixops.mix_clips_host(x, plan)
    assert _bytes_equal(got, expected)
    assert not np.isnan(got[0]).any()


@pytest.mark.parametrize("shape", mc.CLIP_SHAPES, ids=str)
def test_mixup_against_fp64_within_the_counted_roundings(shape):
    """|got - ref| <= 4 * 2^-24 (|lam a| + |(1 - lam) q|): 1 - lam, its product with q and the fused multiply-add are three
    fp32 roundings, plus one (the rule of tests/test_ops_gpu.py)."""
    _lib()
    B, P, H, W = shape
    x = mc.normals(shape, 21)
    for lam in (0.0, 0.25, 0.3, 0.9999999, 1e-3):
        plan = mc.make_plan(B, lam=lam)
        got = mixops.mix_clips_host(x, plan).astype(np.float64)
        ref, mag = mix_ref.mix_clips_fp64(x, plan)
        assert not np.isnan(ref).any()
        assert np.all(np.abs(got - ref) <= 4 * U * mag)


# -- the targets ---------------------------------------------------------------------------------------------------------------
TARGET_CASES = mc.target_cases()


@pytest.mark.parametrize("name,labels,plan,C,sm", TARGET_CASES, ids=[c[0] for c in TARGET_CASES])
def test_targets_host_equals_the_restatement_and_fp64(name, labels, plan, C, sm):
    """Byte for byte against the restatement; against fp64 within 7 * 2^-24 of the terms' magnitude: `on` carries three
    roundings (off, 1 - smoothing, their sum), 1 - lam one, its product one, the fused multiply-add one, plus one."""
    _lib()
    got = mixops.mix_targets_host(labels, plan, C, sm)
    assert _bytes_equal(got, mix_ref.targets(labels, plan, C, sm))
    ref, mag = mix_ref.targets_fp64(labels, plan, C, sm)
    assert np.all(np.abs(got.astype(np.float64) - ref) <= 7 * U * mag)


@pytest.mark.parametrize("C", mc.TARGET_CLASSES)
def test_targets_one_hot_rows_and_labels_outside_the_classes(C):
    _lib()
    labels = np.array([0, C - 1, C // 2, -1, C, 1 << 40], dtype=np.int64)
    B = labels.size
    ident = mc.make_plan(B, partner=np.arange(B), lam=1.0)
    got = mixops.mix_targets_host(labels, ident, C, 0.0)
    want = np.zeros((B, C), dtype=F32)
    for b in range(3):
        want[b, labels[b]] = 1.0
    assert _bytes_equal(got, want)                          # exact one-hot rows; an outside label: an all-off (zero) row
    got = mixops.mix_targets_host(labels, ident, C, 0.1)
    on, off = mix_ref.smooth_rule(0.1, C)
    assert np.all(got[3:] == off) and all(got[b, labels[b]] == on for b in range(3))
    # a partner whose label is outside: its share goes to no class
    mixed = mixops.mix_targets_host(labels, mc.make_plan(B, partner=[3] * B, lam=0.25), C, 0.0)
    assert mixed[0, 0] == F32(0.25) and mixed[0].sum() == F32(0.25)


# -- the soft-target cross entropy ---------------------------------------------------------------------------------------------
CE_CASES = mc.ce_cases()


def torch_soft_ce_fp64(z, t, gs):
    z64 = torch.from_numpy(z.astype(np.float64)).requires_grad_(True)
    loss = F.cross_entropy(z64, torch.from_numpy(t.astype(np.float64)))
    (g,) = torch.autograd.grad(loss, z64)
    return float(loss.detach()), (g * gs).numpy()


def check_soft_ce(loss, dlog, z, t, gs):
    """The project's bounds for head_bce: the loss within 2e-6 relative (exactly 0 at C = 1), the gradient within 2e-6 of its
    largest reference magnitude -- plus the floor of the fp32 format itself, which a softmax row needs and a sigmoid does
    not: with a hard label on a logit of 100 EVERY entry of the row's gradient lies among fp32's subnormals (1e-44), where
    no fp32 value is closer than 2^-150 to the exact one.  expf(z - m) is rounded there (2^-150), so is the quotient by
    s >= 1 (2^-150); St multiplies both; the product with grad_scale / R <= 1 is rounded once more (2^-150): at most
    (2 St + 1) 2^-150 <= (1 + max St) 2^-149.  Against the gradients of every other case (1e-4 and up) the floor is nothing."""
    ref_loss, ref_d = torch_soft_ce_fp64(z, t, gs)
    if z.shape[1] == 1:
        assert float(loss) == 0.0
    assert abs(float(loss) - ref_loss) <= 2e-6 * abs(ref_loss)
    floor = (1.0 + float(np.abs(t.astype(np.float64)).sum(axis=1).max())) * 2.0 ** -149
    err, top = np.abs(dlog.astype(np.float64) - ref_d).max(), np.abs(ref_d).max()
    print("soft_ce R%d C%d gs %g: loss %.9g ref %.9g, gradient error %.3g of max %.3g" % (z.shape + (gs, float(loss), ref_loss,
                                                                                           err, top)))
    assert err <= 2e-6 * top + floor


@pytest.mark.parametrize("name,z,t,gs", CE_CASES, ids=[c[0] for c in CE_CASES])
def test_soft_ce_host_matches_torch_fp64(name, z, t, gs):
    _lib()
    loss, dlog = mixops.soft_ce_host(z, t, gs)
    check_soft_ce(loss[0], dlog, z, t, gs)
    ref_loss, ref_d = mix_ref.soft_ce(z, t, gs)              # the restatement says what torch says
    t_loss, t_d = torch_soft_ce_fp64(z, t, gs)
    assert abs(ref_loss - t_loss) <= 1e-12 * max(1.0, abs(t_loss)) and np.abs(ref_d - t_d).max() <= 1e-12


def test_soft_ce_host_rows_that_do_not_sum_to_one_and_the_draw_counter():
    _lib()
    z = mc.ce_logits(5, 257, 801)
    t = (mc.ce_targets(5, 257, 0.3, 0.1, 802) * np.array([[0.0], [0.5], [1.0], [2.0], [3.5]], dtype=F32)).astype(F32)
    rng = np.array([123, 9], dtype=np.uint64)
    loss, dlog = mixops.soft_ce_host(z, t, 0.25, rng=rng)
    check_soft_ce(loss[0], dlog, z, t, 0.25)
    assert rng.tolist() == [123, 10]
    again = mixops.soft_ce_host(z, t, 0.25)
    assert _bytes_equal(again[0], loss) and _bytes_equal(again[1], dlog)


# -- the BatchMixer's plans -----------------------------------------------------------------------------------------------------
def _plans(mixer, n, B=8, H=79, W=79):
    return [mixer.draw(B, H, W) for _ in range(n)]


@pytest.mark.parametrize("kw", [dict(mixup_alpha=0.8), dict(cutmix_alpha=1.0), dict(mixup_alpha=0.8, cutmix_alpha=1.0),
                                dict(mixup_alpha=0.8, cutmix_alpha=1.0, per_sample=True, prob=0.7)], ids=str)
def test_batch_mixer_plans(kw):
    _lib()
    a = _plans(mixing.BatchMixer(400, seed=5, **kw), 40)
    b = _plans(mixing.BatchMixer(400, seed=5, **kw), 40)
    c = _plans(mixing.BatchMixer(400, seed=6, **kw), 40)
    assert all(_bytes_equal(p, q) for p, q in zip(a, b))                    # the same seed: the same plans
    assert not all(_bytes_equal(p, q) for p, q in zip(a, c))
    H = W = 79
    cut = mix = 0
    for plan in a:
        assert sorted(plan["partner"].tolist()) == list(range(8))           # a permutation
        assert np.all((plan["lam"] >= 0) & (plan["lam"] <= 1))
        if not kw.get("per_sample"):
            assert len({p.tobytes()[4:] for p in plan}) == 1                # one draw per batch
        for e in plan:
            y0, y1, x0, x1 = (int(e[k]) for k in ("y0", "y1", "x0", "x1"))
            if y0 < y1 and x0 < x1:
                cut += 1
                assert 0 <= y0 and y1 <= H and 0 <= x0 and x1 <= W          # inside the plane
                assert e["lam"] == F32(1.0 - (y1 - y0) * (x1 - x0) / float(H * W))
            else:
                assert (y0, y1, x0, x1) == (0, 0, 0, 0)
                mix += e["lam"] != 1
    assert (cut > 0) == ("cutmix_alpha" in kw) and (mix > 0) == ("mixup_alpha" in kw)


def test_batch_mixer_identity_plans_and_refusals():
    _lib()
    for m in (mixing.BatchMixer(400, mixup_alpha=0.8, cutmix_alpha=1.0, prob=0.0), mixing.BatchMixer(400, label_smoothing=0.1)):
        for plan in _plans(m, 5):
            assert np.all(plan["lam"] == 1) and all(int(e[k]) == 0 for e in plan for k in ("y0", "y1", "x0", "x1"))
    assert not mixing.BatchMixer(400, label_smoothing=0.1).mixes
    # a box that comes out empty (lam so close to 1 that int(H * sqrt(1 - lam)) is 0) degrades to the identity
    m = mixing.BatchMixer(10, cutmix_alpha=1e-3, seed=3)
    plans = _plans(m, 200, B=2, H=4, W=4)
    assert any(np.all(p["lam"] == 1) and np.all(p["y1"] == 0) for p in plans)
    for kw in (dict(n_classes=0), dict(n_classes=4, mixup_alpha=-1.0), dict(n_classes=4, cutmix_alpha=float("nan")),
               dict(n_classes=4, prob=1.5), dict(n_classes=4, switch_prob=-0.1), dict(n_classes=4, label_smoothing=1.0)):
        with pytest.raises(ValueError):
            mixing.BatchMixer(**kw)
    with pytest.raises(ValueError):
        m.draw(0, 4, 4)
    with pytest.raises(ValueError):
        m(torch.zeros(2, 3, 4, 8, 8), torch.zeros(2, dtype=torch.int64))   # CPU clips: no fallback


def test_batch_mixer_with_both_alphas_zero_returns_the_clips_themselves(monkeypatch):
    """No clip launch: x comes back as the same object.  The launches are replaced by recorders here (no GPU): mix_targets is
    asked for once, with the smoothing; mix_clips never."""
    _lib()
    calls = []
    monkeypatch.setattr(mixing.mixops, "mix_targets", lambda y, plan, C, sm, out=None: calls.append(("t", C, sm)) or "T")
    monkeypatch.setattr(mixing.mixops, "mix_clips", lambda *a, **k: calls.append(("c",)))
    m = mixing.BatchMixer(400, label_smoothing=0.1)
    monkeypatch.setattr(m, "_upload", lambda plan, dev: plan)
    monkeypatch.setattr(m, "_check", lambda x, y: None)        # host tensors stand for the device's: nothing is launched
    x, y = torch.zeros(2, 3, 4, 8, 8), torch.zeros(2, dtype=torch.int64)
    got_x, got_t = m(x, y)
    assert got_x is x and got_t == "T" and calls == [("t", 400, 0.1)]
    assert np.all(m.last_plan["lam"] == 1)


def test_the_script_defaults_keep_the_hard_label_objective():
    import train_x3d_kinetics_multigrid as script
    sig = inspect.signature(script.run).parameters
    names = ("mixup", "cutmix", "mix_prob", "mix_switch_prob", "label_smoothing")
    assert not script.mixing_on(**{k: sig[k].default for k in names})
    for kw in (dict(mixup=0.8), dict(cutmix=1.0), dict(mix_prob=0.5), dict(mix_switch_prob=0.5), dict(label_smoothing=0.1)):
        assert script.mixing_on(**kw)
    src = open(script.__file__).read()
    for flag, default in (("--mixup", "0.0"), ("--cutmix", "0.0"), ("--mix-prob", "None"), ("--mix-switch-prob", "None"),
                          ("--label-smoothing", "0.0")):
        assert re.search(r"add_argument\('%s', type=float, default=%s," % (flag, default), src), flag


# -- refusals of the wrappers (nothing is launched: no GPU here) -------------------------------------------------------------------
def test_wrappers_refuse_bad_calls_before_anything_is_launched():
    _lib()
    x, plan = torch.zeros(2, 3, 4, 8, 8), torch.zeros(2, 32, dtype=torch.uint8)
    with pytest.raises(ValueError):
        mixops.mix_clips(x, plan)                                          # CPU clips
    with pytest.raises(ValueError):
        mixops.mix_clips(x.double(), plan)
    with pytest.raises(ValueError):
        mixops.mix_clips(x[0, 0], plan)                                    # fewer than 4 dimensions
    with pytest.raises(ValueError):
        mixops.mix_targets(torch.zeros(2, dtype=torch.int64), plan, 400)   # CPU labels
    with pytest.raises(ValueError):
        mixops.mix_targets(torch.zeros(2, dtype=torch.int32), plan, 400)
    z = torch.zeros(2, 4)
    for bad in ((z, z.double()), (z, torch.zeros(2, 5)), (z.view(-1), z.view(-1)), (z, z), ("z", z)):
        with pytest.raises(ValueError):
            mixops.soft_ce(*bad)                                           # the last but one: CPU tensors, no fallback
    with pytest.raises(ValueError):
        mixops.mix_clips_host(np.zeros((2, 3, 4, 4), F32), mixops.identity_plan(3))
    a = np.zeros((2, 3, 4, 4), F32)
    with pytest.raises(_mixlib.X3DHipError):
        mixops.mix_clips_host(a, mixops.identity_plan(2), out=a)            # in place: the library refuses


# -- the sanitised stand-alone program -----------------------------------------------------------------------------------------------
def test_mix_check_program_under_sanitizers(tmp_path):
    """tests/mix_check.cpp with csrc_mix/mix_host.cpp under -fsanitize=address,undefined, as a program of its own: the clip and
    target case lists against the restatement's bytes, the NaN cases, cross-entropy cases against the twin's result as this
    process computed it, and the refusals."""
    _lib()
    recs = [mix_program.clips_record(x, plan, mix_ref.mix_clips(x, plan)) for _, x, plan in CLIP_CASES]
    recs += [mix_program.clips_record(x, plan, want) for _, x, plan, want in NAN_CASES]
    recs += [mix_program.targets_record(lab, plan, C, sm, mix_ref.targets(lab, plan, C, sm)) for _, lab, plan, C, sm in TARGET_CASES]
    n_ce = 0
    for _, z, t, gs in CE_CASES[::6]:
        loss, dlog = mixops.soft_ce_host(z, t, gs)
        recs.append(mix_program.soft_ce_record(z, t, gs, loss, dlog))
        n_ce += 1
    words, _ = mix_program.run(tmp_path, recs)
    assert words == ["ok", str(len(CLIP_CASES) + len(NAN_CASES)), str(len(TARGET_CASES)), str(n_ce)]
