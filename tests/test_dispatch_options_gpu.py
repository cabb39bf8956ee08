"""Exact tests under every dispatch option (GPU): the fallback kernels and the tile / group / grid geometries behind the 29
run-time options of the library (x3d_set_option), `torch.equal` against fp64 like tests/test_exact_gpu.py.

On the integer inputs of tests/exact_inputs.py every kernel must return the fp64 result bit for bit in ANY summation order
(tests/test_exact_inputs_host.py proves it for every case used here), so every option value must pass the same comparison: no
tolerance in this file.  Next to the comparison every test asserts that its setting really changed what runs -- the kernel
name (`_lib.last_kernel()`) or a tile / group query differs from its value under defaults; where no query shows the change
(dw_balance, dw_no_v2, dw_cpb_max, pw_pgrid, pw_two_tiles_k) the case is picked by arithmetic, written next to it.

OPTION_TESTS maps every option to the tests that set it; test_every_option_has_a_test (host) compares its keys with the
library's own table, so an option added without a test fails there."""
import functools
import importlib
import os

import numpy as np
import pytest
import torch

from tests import exact_inputs as ei
from tests.test_exact_gpu import (BWD_OPTS, _canary_bands_around_every_output, _dev, _dw, _dw_bn_forms, _eq, _pw_backward,  # noqa: F401
                                  _pw_device, _pw_forward, _stem, _to)

gpu = pytest.mark.gpu

_HERE, _EXACT = "tests.test_dispatch_options_gpu", "tests.test_exact_gpu"
OPTION_TESTS = {
    "fb_grid": [(_EXACT, "test_pw_exact_integers_long_item_loops")],
    "pw_pgrid": [(_HERE, "test_pw_fwd_chunked_kernel_long_item_loops"), (_HERE, "test_pw_dgrad_chunked_kernels")],
    "pw_nt4_min": [(_HERE, "test_pw_fwd_streaming_voxel_forms")],
    "pw_no_persist": [(_HERE, "test_pw_fwd_tiled_kernel_without_persistence")],
    "dw_th": [(_HERE, "test_dw333_tile_geometries"), (_HERE, "test_dw333_bn_forms_under_small_tiles")],
    "dw_balance": [(_HERE, "test_dw333_tile_geometries")],
    "dw_no_v2": [(_HERE, "test_dw333_tile_geometries")],
    "no_pw6": [(_HERE, "test_pw_fwd_chunked_kernel"), (_HERE, "test_pw_fwd_tiled_kernel_without_persistence")],
    "no_pw7": [(_HERE, "test_pw_dgrad_chunked_kernels")],
    "no_pwfs": [(_HERE, "test_pw_fwd_packed_streaming_kernel"), (_HERE, "test_pw_fwd_streaming_voxel_forms")],
    "dgrad_f32": [(_EXACT, "test_pw_exact_integers")],
    "wgrad_f32": [(_EXACT, "test_pw_exact_integers")],
    "bwd_terms": [(_EXACT, "test_pw_exact_integers"), (_HERE, "test_pw_dgrad_chunked_kernels")],
    "no_wgrad4": [(_HERE, "test_pw_wgrad_narrow_tiles_in_the_batch")],
    "wg_cpw": [(_HERE, "test_pw_wgrad_group_plans")],
    "wg_cap": [(_HERE, "test_pw_wgrad_group_plans")],
    "stem_wg_cap": [(_HERE, "test_stem_wgrad_group_caps")],
    "dw_tsplit_wgs": [(_EXACT, "test_dw333_exact_integers_t_segments"), (_HERE, "test_dw333_tile_geometries")],
    "dw_cpb_max": [(_HERE, "test_dw333_tile_geometries"), (_HERE, "test_dw333_bn_forms_under_small_tiles")],
    "pw6_min_m": [(_HERE, "test_pw_fwd_whole_k_kernels_at_three_m_tiles")],
    "pw_two_tiles_k": [(_HERE, "test_pw_whole_k_tiles_per_wave")],
    "dw_tsplit_wgs_fwd": [(_EXACT, "test_dw333_exact_integers_t_segments"), (_HERE, "test_dw333_tile_geometries")],
    "no_pw8": [(_EXACT, "test_pw_exact_integers_sixteen_wave_modes"), (_HERE, "test_pw_fwd_chunked_kernel")],
    "pw8_grid": [(_EXACT, "test_pw_exact_integers_long_item_loops")],
    "pw8_max_k": [(_EXACT, "test_pw_exact_integers_long_item_loops")],
    "no_se_bwd_merge": [(_EXACT, "test_elementwise_bn_se_operands_as_flat_buffer_views")],
    "pw_waves16": [(_EXACT, "test_pw_exact_integers_sixteen_wave_modes"), (_HERE, "test_pw_whole_k_tiles_per_wave")],
    "dw_tquad_wgs": [(_EXACT, "test_dw333_exact_integers_t_segments")],
    "dw_tquad_wgs_fwd": [(_EXACT, "test_dw333_exact_integers_t_segments")],
}


def test_every_option_has_a_test():
    """Host: the keys of OPTION_TESTS are exactly the library's option table (x3d_option_count / x3d_option_name), and every
    test the table names exists in the module it names."""
    from x3dhip import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as ge
        ge.build()
    L = _lib.lib()
    names = [L.x3d_option_name(i).decode() for i in range(L.x3d_option_count())]
    assert len(names) == len(set(names)) == 29
    assert sorted(OPTION_TESTS) == sorted(names), (sorted(set(names) - set(OPTION_TESTS)), sorted(set(OPTION_TESTS) - set(names)))
    for opt, tests in OPTION_TESTS.items():
        assert tests, opt
        for module, test in tests:
            assert callable(getattr(importlib.import_module(module), test, None)), (opt, module, test)


# ------------------------------------------------------------------------------------------------- shared pieces
@functools.lru_cache(maxsize=3)
def _pw(case):
    """(inputs, fp64 reference) of a pointwise case: computed once, shared by the tests that use the case, never modified."""
    c = ei.pw_case(case)
    return c, ei.pw_ref(c)


@functools.lru_cache(maxsize=2)
def _dwc(case):
    c = ei.dw_case(case)
    return c, ei.dw_ref(c)


def _fwd_kernel(ops, _lib, c, d):
    """The kernel a packed forward of this case lands on under the options set NOW."""
    ops.pw_fwd(d["x"], d["w"], stride=c.s, pre=d["pre"], pre_act=c.act, wp=ops.pw_pack(d["w"]))
    return _lib.last_kernel()


def _dgrad_kernel(ops, _lib, d):
    ops.pw_bwd_data(d["g"], d["a"], d["cb"], d["w"], wpt=ops.pw_pack(d["w"], transposed=True))
    return _lib.last_kernel()


def _P(case):
    N, Ci, Co, T, H, W, s, act = case
    return T * ei.out_hw(H, s) * ei.out_hw(W, s)


# ------------------------------------------------------------------------------------------------- 1. pointwise forward
_PW4 = dict(no_pw8=1, no_pw6=1)


@gpu
@pytest.mark.parametrize("case", ei.PW_OPT_DENSE)
def test_pw_fwd_chunked_kernel(case):
    """no_pw8 + no_pw6: the chunked persistent kernel pw4_kernel (IN_FWD with the statistics epilogue; by default only
    K > 448) on the stage 3-4 widths: 14 M tiles in two blocks (U = 4), 12 in two (U = 3), 6 in one (U = 3)."""
    from x3dhip import _lib, ops
    dev = _dev()
    c, r = _pw(case)
    d = _pw_device(c, dev)
    assert _fwd_kernel(ops, _lib, c, d) in ("pw6_kernel", "pw8_kernel")
    with _lib.options(**_PW4):
        _pw_forward(ops, c, r, d, "%s %s" % (case, _PW4))
        assert _lib.last_kernel() == "pw4_kernel", _lib.last_kernel()


@gpu
@pytest.mark.parametrize("grid", [3, 40])
def test_pw_fwd_chunked_kernel_long_item_loops(grid):
    """pw4_kernel on 3 / 40 workgroups (pw_pgrid): 32 items (2 samples x 8 voxel tiles x 2 M blocks) and 48 items (3 x 8 x 2)
    -- default: one item per workgroup; here 11 and 16 items per workgroup on 3, and 48 items on 40 (a second round of 8)."""
    from x3dhip import _lib, ops
    dev = _dev()
    with _lib.options(pw_pgrid=grid, **_PW4):
        for case in ei.PW_GRID[:2]:
            c, r = _pw(case)
            _pw_forward(ops, c, r, _pw_device(c, dev), "%s pw_pgrid %d" % (case, grid))
            assert _lib.last_kernel() == "pw4_kernel", _lib.last_kernel()


@gpu
@pytest.mark.parametrize("case", ei.PW_OPT_DENSE)
def test_pw_fwd_tiled_kernel_without_persistence(case):
    """pw_no_persist (+ no_pw6, no_pw8): the LDS-tiled pw2_kernel in its float4 form -- by default dense shapes never reach it.
    M blocks of 7, 4 and 6 tiles (both `mt_run > 4` builds)."""
    from x3dhip import _lib, ops
    dev = _dev()
    c, r = _pw(case)
    d = _pw_device(c, dev)
    opts = dict(pw_no_persist=1, **_PW4)
    with _lib.options(**opts):
        _pw_forward(ops, c, r, d, "%s %s" % (case, opts))
        assert _lib.last_kernel() == "pw2_kernel", _lib.last_kernel()
    with _lib.options(**_PW4):
        assert _fwd_kernel(ops, _lib, c, d) == "pw4_kernel"               # what the same shape runs on without the option


@gpu
@pytest.mark.parametrize("case", ei.PW_OPT_STREAM)
def test_pw_fwd_packed_streaming_kernel(case):
    """no_pwfs: pw3_kernel on the stage 1-2 shapes.  The expanding convs (M >= K) run on pw_fwd_stream_kernel by default, the
    contracting one is on pw3 either way."""
    from x3dhip import _lib, ops
    dev = _dev()
    N, Ci, Co = case[:3]
    c, r = _pw(case)
    d = _pw_device(c, dev)
    L = _lib.lib()
    default = _fwd_kernel(ops, _lib, c, d)
    assert default == ("pw_fwd_stream_kernel" if Co >= Ci else "pw3_kernel"), default
    tiles = L.x3d_pw_fwd_tiles(N, Ci, Co, _P(case), 1, 1)
    with _lib.options(no_pwfs=1):
        _pw_forward(ops, c, r, d, "%s no_pwfs" % (case,))
        assert _lib.last_kernel() == "pw3_kernel", _lib.last_kernel()
        if Co >= Ci:
            assert L.x3d_pw_fwd_tiles(N, Ci, Co, _P(case), 1, 1) != tiles


# pw_plan's streaming forms: (case, pw_nt4_min) -> tiles of x3d_pw_tiles.  16-voxel waves give cdiv(P, 64) tiles, the float4
# form cdiv(P, 256).  Defaults: 4 (2 workgroups < 256), 391 (196 < 256), 98 (294 >= 256)
_NT4 = [((2, 24, 54, 4, 8, 8, 1, 0), 0, 1, 4), ((2, 24, 54, 4, 79, 79, 1, 1), 1 << 30, 391, 391), ((2, 24, 54, 4, 79, 79, 1, 1), 0, 98, 391),
        ((3, 24, 54, 4, 79, 79, 1, 1), 1 << 30, 391, 98)]


@gpu
@pytest.mark.parametrize("case,nt4_min,tiles,default_tiles", _NT4)
def test_pw_fwd_streaming_voxel_forms(case, nt4_min, tiles, default_tiles):
    """pw_nt4_min = 0 / 2^30: the float4 and the 16-voxel form of the streaming kernels, unpacked (pw_kernel) and packed under
    no_pwfs (pw3_kernel).  (2, ..., 79, 79) is on the 16-voxel form by default: there only pw_nt4_min = 0 changes the launch;
    with three samples the default is the float4 form and 2^30 changes it."""
    from x3dhip import _lib, ops
    dev = _dev()
    N, Ci, Co = case[:3]
    c, r = _pw(case)
    d = _pw_device(c, dev)
    L = _lib.lib()
    assert L.x3d_pw_tiles(N, Ci, Co, _P(case), 1) == default_tiles
    with _lib.options(pw_nt4_min=nt4_min, no_pwfs=1):
        assert L.x3d_pw_tiles(N, Ci, Co, _P(case), 1) == tiles
        ops.pw_fwd(d["x"], d["w"], pre=d["pre"], pre_act=c.act)
        assert _lib.last_kernel() == "pw_kernel", _lib.last_kernel()
        _pw_forward(ops, c, r, d, "%s pw_nt4_min %d" % (case, nt4_min))
        assert _lib.last_kernel() == "pw3_kernel", _lib.last_kernel()


@gpu
@pytest.mark.parametrize("case", ei.PW_OPT_FLOAT4)
def test_pw_streaming_float4_form_both_directions(case):
    """pw_nt4_min = 0 (+ no_pwfs): the float4 form of pw_kernel and pw3_kernel, forward and every data-gradient epilogue
    (plain / ReLU backward / residual-mask backward; no, dense and stride-2 addend).  By default the form needs 256 workgroups
    of 256 voxels, and the exact cases that large have 54 output rows forward only.  Here: one 256-voxel tile per sample, M
    blocks of four tiles (-> 54 rows) and of two (-> 24), raw and activated input."""
    from x3dhip import _lib, ops
    dev = _dev()
    N, Ci, Co = case[:3]
    c, r = _pw(case)
    d = _pw_device(c, dev)
    L = _lib.lib()
    assert L.x3d_pw_tiles(N, Ci, Co, _P(case), 1) == 4                      # 16-voxel waves: cdiv(256, 64)
    with _lib.options(pw_nt4_min=0, no_pwfs=1):
        assert L.x3d_pw_tiles(N, Ci, Co, _P(case), 1) == L.x3d_pw_tiles(N, Co, Ci, _P(case), 1) == 1
        ops.pw_fwd(d["x"], d["w"], pre=d["pre"], pre_act=c.act)
        assert _lib.last_kernel() == "pw_kernel", _lib.last_kernel()
        _pw_forward(ops, c, r, d, "%s pw_nt4_min 0" % (case,))
        assert _lib.last_kernel() == "pw3_kernel", _lib.last_kernel()
        assert _dgrad_kernel(ops, _lib, d) == "pw3_kernel"
        _pw_backward(ops, c, r, d, "%s pw_nt4_min 0" % (case,))


@gpu
@pytest.mark.parametrize("case", ei.PW_OPT_DGRAD + ei.PW_OPT_DENSE[1:2])
def test_pw_tiled_kernel_without_persistence_both_directions(case):
    """pw_no_persist + no_pw6 / no_pw7 / no_pw8: pw2_kernel's float4 form forward and on every data-gradient epilogue -- M
    blocks of 7, 4 and 6 tiles for the first three data gradients and 4 behind the activated 432 -> 192 (both `mt_run > 4`
    builds with and without the ReLU backward); forward 192 -> 432 is the raw input on blocks of 4."""
    from x3dhip import _lib, ops
    dev = _dev()
    c, r = _pw(case)
    d = _pw_device(c, dev)
    opts = dict(pw_no_persist=1, no_pw7=1, **_PW4)
    with _lib.options(**opts):
        _pw_forward(ops, c, r, d, "%s %s" % (case, opts))
        assert _lib.last_kernel() == "pw2_kernel", _lib.last_kernel()
        assert _dgrad_kernel(ops, _lib, d) == "pw2_kernel"
        _pw_backward(ops, c, r, d, "%s %s" % (case, opts))


@gpu
def test_pw_tiled_kernel_element_loads_raw_input():
    """Defaults: 96 -> 216 at P = 98 (P % 4 != 0) is outside the whole-K and the chunked kernels: pw2_kernel's element-load form
    with a raw input and two M tiles per wave forward, its three data-gradient epilogues backward."""
    from x3dhip import _lib, ops
    dev = _dev()
    case = ei.PW_OPT_TILED[0]
    c, r = _pw(case)
    d = _pw_device(c, dev)
    _pw_forward(ops, c, r, d, "%s" % (case,))
    assert _lib.last_kernel() == "pw2_kernel", _lib.last_kernel()
    assert _dgrad_kernel(ops, _lib, d) == "pw2_kernel"
    _pw_backward(ops, c, r, d, "%s" % (case,))


@gpu
@pytest.mark.parametrize("no_pw8,kernel", [(1, "pw6_kernel"), (0, "pw8_kernel")])
def test_pw_fwd_whole_k_kernels_at_three_m_tiles(no_pw8, kernel):
    """pw6_min_m = 16: K = 108 -> M = 48 on the whole-K kernels (five of the eight waves own no M tile); default: pw3."""
    from x3dhip import _lib, ops
    dev = _dev()
    case = ei.PW_OPT_WHOLE_K[0]
    c, r = _pw(case)
    d = _pw_device(c, dev)
    assert _fwd_kernel(ops, _lib, c, d) == "pw3_kernel"
    with _lib.options(pw6_min_m=16, no_pw8=no_pw8):
        _pw_forward(ops, c, r, d, "%s pw6_min_m 16 no_pw8 %d" % (case, no_pw8))
        assert _lib.last_kernel() == kernel, _lib.last_kernel()


@gpu
@pytest.mark.parametrize("two_tiles_k", [32, 4096])
def test_pw_whole_k_tiles_per_wave(two_tiles_k):
    """pw_two_tiles_k with pw_waves16 = 0, no_pw8 = 1 (the 8-wave pw6 / pw7).  No query shows the M blocking; by arithmetic
    (x3d_pw6_launch, x3d_pw7_launch: 16 tiles per block from kp >= pw_two_tiles_k, else 8):
    32:   forward 96 -> 216 (kp = 96): 14 M tiles in ONE block, two per wave (default: two blocks of 7);
          data gradient of 432 -> 192 (kp = 192, M = 432): 27 tiles in two blocks of 14 (default: four of 7);
    4096: forward 432 -> 192 (kp = 448): 12 M tiles in two blocks of 6 (default: one block, two per wave)."""
    from x3dhip import _lib, ops
    dev = _dev()
    with _lib.options(pw_two_tiles_k=two_tiles_k, pw_waves16=0, no_pw8=1):
        for case in ei.PW_OPT_DENSE[:2]:
            c, r = _pw(case)
            d = _pw_device(c, dev)
            what = "%s pw_two_tiles_k %d" % (case, two_tiles_k)
            _pw_forward(ops, c, r, d, what)
            assert _lib.last_kernel() == "pw6_kernel", _lib.last_kernel()
            assert _dgrad_kernel(ops, _lib, d) == "pw7_kernel"
            _pw_backward(ops, c, r, d, what)


@gpu
@pytest.mark.parametrize("case", ei.PW_XL)
def test_pw_xl_widths(case):
    """X3D-XL's 630 channels under defaults: 280 -> 630 is pw6 with 40 M tiles forward and the chunked pw4 (three terms) /
    pw5 (two terms) backward (K = 630 is beyond pw7's LDS tile); 630 -> 280 is pw4 forward and pw7 backward.  The P = 50 cases
    (P % 4 != 0) take the element-load forms."""
    from x3dhip import _lib, ops
    dev = _dev()
    N, Ci, Co = case[:3]
    c, r = _pw(case)
    d = _pw_device(c, dev)
    if _P(case) % 4 == 0:
        assert _fwd_kernel(ops, _lib, c, d) == ("pw6_kernel" if Ci == 280 else "pw4_kernel")
        assert _dgrad_kernel(ops, _lib, d) == ("pw4_kernel" if Ci == 280 else "pw7_kernel")
        if Ci == 280:
            with _lib.options(bwd_terms=2):
                assert _dgrad_kernel(ops, _lib, d) == "pw5_kernel"
    _pw_forward(ops, c, r, d, "%s" % (case,))
    for opts in BWD_OPTS:
        with _lib.options(**opts):
            _pw_backward(ops, c, r, d, "%s %s" % (case, opts))


# ------------------------------------------------------------------------------------------------- 2. data gradient
@gpu
@pytest.mark.parametrize("pgrid", [512, 3])
@pytest.mark.parametrize("terms,kernel", [(3, "pw4_kernel"), (2, "pw5_kernel")])
@pytest.mark.parametrize("case", ei.PW_OPT_DGRAD)
def test_pw_dgrad_chunked_kernels(case, terms, kernel, pgrid):
    """no_pw7: the data gradient (plain, addend, stride-2 addend, the three pw_bwd_data_res forms) on the chunked persistent
    kernels -- pw4_kernel with three-term operands, pw5_kernel with two -- also on 3 workgroups (pw_pgrid: 32 ... 48 items)."""
    from x3dhip import _lib, ops
    dev = _dev()
    N, Ci, Co = case[:3]
    c, r = _pw(case)
    d = _pw_device(c, dev)
    L = _lib.lib()
    default = _dgrad_kernel(ops, _lib, d)
    assert default == "pw7_kernel", default
    tiles = L.x3d_pw_bwd_tiles(N, Ci, Co, _P(case), 1, 0)
    opts = dict(no_pw7=1, bwd_terms=terms, pw_pgrid=pgrid)
    with _lib.options(**opts):
        assert L.x3d_pw_bwd_tiles(N, Ci, Co, _P(case), 1, 0) != tiles
        assert _dgrad_kernel(ops, _lib, d) == kernel
        _pw_backward(ops, c, r, d, "%s %s" % (case, opts))


# ------------------------------------------------------------------------------------------------- 3. weight gradient
def _wgrad(ops, _lib, c, r, d, what):
    """Single launch and the batched launch behind DeferredGrads; returns the two kernel names."""
    N, Ci, Co = c.shape[:3]
    dw = ops.pw_bwd_weight(d["g"], d["a"], d["cb"], d["x"], (Co, Ci), stride=c.s, pre=d["pre"], pre_act=c.act)
    k1 = _lib.last_kernel()
    _eq(dw, r["dw"], what + " pw_bwd_weight")
    df = ops.DeferredGrads()
    dw = ops.pw_bwd_weight(d["g"], d["a"], d["cb"], d["x"], (Co, Ci), stride=c.s, pre=d["pre"], pre_act=c.act, defer=df)
    df.flush()
    k2 = _lib.last_kernel()
    _eq(dw, r["dw"], what + " pw_bwd_weight through DeferredGrads")
    return k1, k2


# x3d_pw_wgrad_groups of wgrad_plan: min(cdiv(chunks, wg_cpw), max(wg_cap / blocks, 16)) & ~7 from 8 on.
# (20, 96, 112, 8, 14, 14): 500 chunks of 64 voxels (25 per sample, the last one half empty), 2 blocks; default 56 groups.
# (2, 48, 96, 4, 16, 16) stride 2 (the gathered kernel): 8 chunks, 1 block; default 1 group.
_WG_PLANS = [(dict(wg_cpw=1), 128, 8),                       # capped
             (dict(wg_cpw=1, wg_cap=65535), 496, 8),         # 496 groups for 500 chunks: four groups walk a second chunk
             (dict(wg_cpw=3), 128, 3),
             (dict(wg_cpw=4096), 1, 1),                      # one workgroup walks every chunk of every sample
             (dict(wg_cap=1), 16, 1)]                        # the floor of 16 groups: 31-32 chunks per workgroup


@gpu
@pytest.mark.parametrize("which", [0, 1])
def test_pw_wgrad_group_plans(which):
    """wg_cpw / wg_cap: the tiled weight gradient, single launch and batched, on every group count of _WG_PLANS -- the cap, the
    floor, the uneven split left by `& ~7`, and one workgroup that walks all chunks across the sample boundaries."""
    from x3dhip import _lib, ops
    dev = _dev()
    case = ei.PW_OPT_WGRAD[which]
    N, Ci, Co, T, H, W, s, act = case
    c, r = _pw(case)
    d = _pw_device(c, dev)
    L = _lib.lib()
    default = L.x3d_pw_wgrad_groups(N, _P(case), Co, Ci, s)
    assert default == (56, 1)[which]
    changed = 0
    for opts, g0, g1 in _WG_PLANS:
        want = (g0, g1)[which]
        with _lib.options(**opts):
            assert L.x3d_pw_wgrad_groups(N, _P(case), Co, Ci, s) == want, opts
            k = _wgrad(ops, _lib, c, r, d, "%s %s" % (case, opts))
        assert k == ("pw_wgrad3_kernel", "pw_wgrad3_batch_kernel"), k
        changed += want != default
    assert changed >= (5, 3)[which]


@gpu
@pytest.mark.parametrize("case,kind", [((2, 96, 216, 4, 10, 10, 1, 0), 1), ((2, 432, 192, 4, 5, 5, 1, 2), 2)])
def test_pw_wgrad_narrow_tiles_in_the_batch(case, kind):
    """no_wgrad4: the batched launch on the 128 x 64 tiles of pw_wgrad3_batch_kernel where the wide tiles (kind 1: 256 x 96,
    kind 2: 128 x 224) run by default."""
    from x3dhip import _lib, ops
    dev = _dev()
    c, r = _pw(case)
    d = _pw_device(c, dev)
    assert _wgrad(ops, _lib, c, r, d, "%s" % (case,))[1] == "pw_wgrad4_batch_kernel"
    with _lib.options(no_wgrad4=1):
        assert _wgrad(ops, _lib, c, r, d, "%s no_wgrad4" % (case,))[1] == "pw_wgrad3_batch_kernel"


# ------------------------------------------------------------------------------------------------- 4. depthwise geometry
# No query shows these three; by the arithmetic of make_geom:
# dw_balance = 0: (4, 216, 2, 40, 40, 1) has tiles of 16 / 16 / 8 rows instead of 14 / 14 / 12, (2, 54, 4, 79, 79, 2) backward
#                 tiles of 12 x 6 + 7 rows either way but forward (40 rows) 16 / 16 / 8 instead of 14 / 14 / 12;
# dw_no_v2 = 1:   W = 10 (2, 216, 4, 10, 10, 1) and Wo = 10 (2, 216, 4, 20, 20, 2) move from float2 to element loads;
# dw_cpb_max:     every case but the 79-wide one has ipc = TH x groups <= 128 in one direction at least and C >= 2, so 3 and 1
#                 channels per workgroup replace 16 ... 2; 1 is the one-channel (uniform-weight) build of both kernels.
_DW_SETTINGS = [dict(dw_th=1), dict(dw_th=2), dict(dw_th=3), dict(dw_th=5), dict(dw_th=7), dict(dw_balance=0), dict(dw_cpb_max=1),
                dict(dw_cpb_max=3), dict(dw_no_v2=1), dict(dw_th=3, dw_balance=0, dw_cpb_max=3)]
_TSPLIT = dict(dw_tsplit_wgs=1 << 20, dw_tsplit_wgs_fwd=1 << 20)


@gpu
@pytest.mark.parametrize("case", ei.DW_OPT)
def test_dw333_tile_geometries(case):
    """dw333_fwd / dw333_bwd (y, dx, dw, both statistics) under every tile height 1 ... 7 (dw_th), unbalanced tiles, 1 and 3
    channels per workgroup, element loads, and one crossed setting (on the T = 8 case with the T march split)."""
    from x3dhip import _lib, ops
    dev = _dev()
    N, C, T, H, W, s = case
    Ho, Wo = ei.out_hw(H, s), ei.out_hw(W, s)
    c, r = _dwc(case)
    d = {k: _to(getattr(c, k), dev) for k in ("x", "w", "pre", "g", "a", "cb")}
    L = _lib.lib()
    fwd0, bwd0 = L.x3d_dw_tiles(N, C, T, Ho, Wo), L.x3d_dw_bwd_tiles(N, C, T, H, W, s)
    for opts in _DW_SETTINGS:
        if len(opts) == 3 and T >= 8:
            opts = dict(opts, **_TSPLIT)
        with _lib.options(**opts):
            fwd, bwd = L.x3d_dw_tiles(N, C, T, Ho, Wo), L.x3d_dw_bwd_tiles(N, C, T, H, W, s)
            if "dw_th" in opts and len(opts) == 1:
                assert (fwd != fwd0) == (Ho > opts["dw_th"]), (opts, fwd, fwd0)
                assert (bwd != bwd0) == (H > opts["dw_th"]), (opts, bwd, bwd0)
            _dw(ops, c, r, d, "%s %s" % (case, opts))


@gpu
@pytest.mark.parametrize("case", [(2, 6, 4, 14, 14, 1), (2, 4, 4, 16, 16, 2)])
def test_dw333_bn_forms_under_small_tiles(case):
    """x3d_dw333_fwd_stats / x3d_dw333_bwd_stats (the BN finalizes folded into the prologues) under dw_th = 3, dw_cpb_max = 3:
    5 and 3 row tiles forward, 5 and 8 backward instead of one, the finalize of three channels per workgroup."""
    from x3dhip import _lib, ops
    dev = _dev()
    N, C, T, H, W, s = case
    L = _lib.lib()
    args = (N, C, T, ei.out_hw(H, s), ei.out_hw(W, s)), (N, C, T, H, W, s)
    assert (L.x3d_dw_tiles(*args[0]), L.x3d_dw_bwd_tiles(*args[1])) == (1, 1)
    with _lib.options(dw_th=3, dw_cpb_max=3):
        assert (L.x3d_dw_tiles(*args[0]), L.x3d_dw_bwd_tiles(*args[1])) == ((5, 5) if s == 1 else (3, 8))
        _dw_bn_forms(ops, case, dev)


@gpu
def test_dw333_bwd_refuses_rows_too_wide_for_an_even_tile():
    """Stride-2 backward needs an even tile height from two row tiles on; W > 512 leaves room for one row per workgroup only:
    the entry point refuses the shape (before this check it read one staged row past the tile's window)."""
    from x3dhip import _lib, ops
    dev = _dev()
    x = torch.zeros(1, 1, 1, 3, 516, device=dev)
    g = torch.zeros(1, 1, 1, 2, 258, device=dev)
    cb = torch.zeros(1, 1, 3, device=dev)
    w = torch.zeros(1, 1, 3, 3, 3, device=dev)
    with pytest.raises(_lib.X3DHipError, match="too wide"):
        ops.dw333_bwd(g, g, cb, w, x, stride=2)


# ------------------------------------------------------------------------------------------------- 5. stem
@gpu
@pytest.mark.parametrize("cap", [1, 5, 7])
def test_stem_wgrad_group_caps(cap):
    """stem_wg_cap: 1, 5 and 7 workgroups walk the tiles of stem133_bwd_weight (64 tiles on 5 groups: range boundaries inside
    planes and rows); defaults: 64, 24 and 80 groups."""
    from x3dhip import _lib, ops
    dev = _dev()
    L = _lib.lib()
    for shape in [(2, 3, 4, 16, 16), (1, 3, 3, 15, 11), (2, 3, 5, 17, 23)]:
        N, _, T = shape[:3]
        assert L.x3d_stem_wgrad_groups(N, T) == N * T * 8 > cap
        with _lib.options(stem_wg_cap=cap):
            assert L.x3d_stem_wgrad_groups(N, T) == cap
            _stem(ops, shape, dev, " stem_wg_cap %d" % cap)


@gpu
@pytest.mark.parametrize("shape,groups,tiles", [((9, 3, 8, 16, 16), 512, 576), ((1, 3, 1, 6, 260), 8, 6), ((1, 3, 2, 5, 259), 16, 12)])
def test_stem_wgrad_cap_and_empty_groups(shape, groups, tiles):
    """Defaults: the cap of 512 groups where N T 8 = 576; Wo = 130: two runs per output row, and more groups than tiles --
    the groups without a tile must still write zeros."""
    from x3dhip import _lib, ops
    dev = _dev()
    N, _, T, H, W = shape
    assert _lib.lib().x3d_stem_wgrad_groups(N, T) == groups
    assert N * T * ei.out_hw(H, 2) * -(-ei.out_hw(W, 2) // 128) == tiles
    _stem(ops, shape, dev)


# ------------------------------------------------------------------------------------------------- 6. engine switches
_COUNTED = ("dw333_fwd", "dw333_fwd_stats", "bn_add_relu_bwd", "se_fwd", "se_bn_fwd", "pw_bwd_fused", "dw333_bwd")


def _golden_step(case, dev, monkeypatch, switch=None, value=None):
    """One training step of a golden case as tests/test_model_gpu.py::test_train_step_vs_reference_golden runs it, with one
    engine switch flipped; the same three checks against the reference's golden vectors.  Returns the number of calls of the
    ops functions a switch brings in or takes out."""
    from tests import parity
    from tests.test_model_gpu import _build
    from x3dhip import engine, ops, synthetic
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", case + ".npz"))
    B, T, H, S = [int(v) for v in g["shape"]]
    calls = dict.fromkeys(_COUNTED + ("dw333_bwd_bn",), 0)
    with monkeypatch.context() as m:
        for name in _COUNTED:
            def counted(*a, _f=getattr(ops, name), _n=name, **kw):
                calls[_n] += 1
                if kw.get("bn") is not None:
                    calls["dw333_bwd_bn"] += 1
                return _f(*a, **kw)
            m.setattr(ops, name, counted)
        prev = getattr(engine.cfg, switch) if switch else None
        if switch:
            setattr(engine.cfg, switch, value)
        try:
            net = _build(case.split("_")[1], S, dev, int(g["seed"][0]))
            net.train(True)
            x = synthetic.synthetic_clips(B, T, H, H, seed=int(g["seed"][1])).to(dev)
            y = synthetic.synthetic_labels(B, seed=int(g["seed"][1])).to(dev)
            logits = net(x)
            loss = torch.nn.CrossEntropyLoss()(logits, y)
            loss.backward()
            torch.cuda.synchronize()
        finally:
            if switch:
                setattr(engine.cfg, switch, prev)
    parity.check_forward(logits.detach().cpu().numpy()[:, :, 0], loss.item(), g)
    grads = {k: p.grad.detach().cpu().numpy() for k, p in net.named_parameters()}
    parity.check_grads(grads, g, synthetic.gradient_sketch, cond=parity.conditioning(case), case=case)      # never pinned
    parity.check_bn_stats({k: v.cpu().numpy() for k, v in net.state_dict().items() if v.ndim}, g)
    return calls


_default_calls = {}


def _defaults(case, dev, monkeypatch):
    if case not in _default_calls:
        _default_calls[case] = _golden_step(case, dev, monkeypatch)
    return _default_calls[case]


@gpu
@pytest.mark.parametrize("switch,value,case", [("no_dw_stats", True, "train_M_8x4x64_s2"), ("no_res_fuse", True, "train_M_8x4x64_s2"),
                                               ("no_se_merge", True, "train_M_8x4x64_s2"), ("no_fused_bwd", True, "train_M_8x4x64_s2"),
                                               ("dw_bwd_stats", False, "train_M_2x4x111_s1")])
def test_engine_schedule_switches_vs_reference_golden(switch, value, case, monkeypatch):
    """Each schedule switch of x3dhip.engine.cfg, one at a time, against the reference's golden vectors with the criteria of
    test_train_step_vs_reference_golden (conditioning-aware bounds, never pinned); the call counts show that the switch
    changed the schedule."""
    dev = _dev()
    d0 = _defaults(case, dev, monkeypatch)
    c = _golden_step(case, dev, monkeypatch, switch, value)
    if switch == "no_dw_stats":
        assert d0["dw333_fwd"] == 0 and d0["dw333_fwd_stats"] > 0
        assert c["dw333_fwd"] == d0["dw333_fwd_stats"] and c["dw333_fwd_stats"] == 0
    elif switch == "no_res_fuse":
        assert c["bn_add_relu_bwd"] == c["dw333_bwd"] > d0["bn_add_relu_bwd"]        # one per block
    elif switch == "no_se_merge":
        assert d0["se_fwd"] == 0 and d0["se_bn_fwd"] > 0
        assert c["se_fwd"] == d0["se_bn_fwd"] and c["se_bn_fwd"] == 0
    elif switch == "no_fused_bwd":
        assert d0["pw_bwd_fused"] > 0 and c["pw_bwd_fused"] == 0
    else:
        assert d0["dw333_bwd_bn"] > 0 and c["dw333_bwd_bn"] == 0
