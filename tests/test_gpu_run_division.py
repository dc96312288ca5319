"""diff / trunc of the one-frame kernel (integrate_tile) through the launch-wide refined reciprocal on wavefronts that took the
fast projection path (csrc/tsdf_kernels.hip.h, integrate_tile_body; fast_div_r).  Every stored bit must stay what the
compiler's division gives: the reference kernel's replay (tests/whole_volume.py) or, for uploaded states, the CPU oracle.

Shapes: 512 x 9 x 6 -- two segments per row, an odd dim_y so that the last pair of rows a lane owns is partial -- whole and
as the slab z [2, 5).  Every comparison is bit for bit."""
import numpy as np
import pytest

import whole_volume as wv
from semantic_slam_amd import capi, synth

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not wv.available(), reason="oracle/_ref/libtsdf_ref_hip.so not built")]

DIMS, VS = (512, 9, 6), 0.005
SLABS = [(0, 6), (2, 5)]
N = 8
_S = {}


def scene(torch):
    """S-band over DIMS, once per session: origin, poses, the constant depth frame and a mask that passes every pixel."""
    if not _S:
        full = synth.sfull_depth()
        _S.update(origin=synth.sband_volume(DIMS, VS), poses=np.stack([synth.sband_pose(k) for k in range(N)]), full=full,
                  full_dev=torch.from_numpy(full).cuda(), pass_all=torch.full(full.shape, 255, dtype=torch.uint8, device="cuda"))
    return _S


def config(zb=0, ze=DIMS[2], trunc=synth.SBAND_TRUNC):
    return capi.make_config(DIMS, VS, _S["origin"], trunc=trunc, z_begin=zb, z_end=ze)


def reference(torch, cfg, k):
    """The reference kernel's replay of the first k S-band frames over the whole grid (cached, shared, never changed)."""
    S = _S
    return wv.replay(torch, f"rundiv_sband_{k}", cfg.cam_K, DIMS, cfg.origin, cfg.voxel_size, cfg.trunc_margin, list(S["poses"][:k]),
                     [S["full_dev"]] * k)


def segments(cfg):
    return 2 * DIMS[1] * (cfg.z_end - cfg.z_begin)


def volume(cfg, variant=None):
    vol = capi.Volume(cfg)
    vol.set_deferral(0)
    if variant is not None:
        vol.set_kernel_variant(variant)
    return vol


def oracle_step(oracle, cfg, pose, depth, t, w):
    oracle.integrate(cfg.cam_K, oracle.cam2base(synth.identity_pose(), pose), depth, DIMS, _S["origin"], VS, cfg.trunc_margin, t, w,
                     z_begin=cfg.z_begin, z_end=cfg.z_end)


def assert_equals_oracle(vol, t, w, what):
    got_t, got_w = vol.download()
    assert np.array_equal(got_w.view(np.uint32), w.view(np.uint32)), f"{what}: weights differ from the oracle"
    bad = np.flatnonzero(got_t.view(np.uint32) != t.view(np.uint32))
    assert bad.size == 0, (f"{what}: {bad.size} TSDF values differ from the oracle; first at {bad[0]}: got "
                           f"0x{got_t.view(np.uint32)[bad[0]]:08x}, oracle 0x{t.view(np.uint32)[bad[0]]:08x}")


@pytest.mark.parametrize("zb,ze", SLABS)
@pytest.mark.parametrize("masked", [False, True], ids=["plain", "masked"])
def test_dense_path_keeps_every_run(cuda, masked, zb, ze):
    """8 S-band frames from a fresh volume: every voxel is inside the band at every launch, so every diff / trunc goes through
    the shared reciprocal (integrate_tile<2, false>, and <2, true> under a mask that passes everything); the rows keep their
    weight runs."""
    S = scene(cuda)
    cfg = config(zb, ze)
    total = segments(cfg)
    with volume(cfg, 7 if masked else None) as vol:
        for k in range(1, N + 1):
            if masked:
                vol.integrate_masked_device(S["full_dev"].data_ptr(), S["pass_all"].data_ptr(), S["poses"][k - 1])
            else:
                vol.integrate_device(S["full_dev"].data_ptr(), S["poses"][k - 1])
            ref_t, ref_w = reference(cuda, cfg, k)
            wv.assert_volume_equals_reference(cuda, f"S-band z [{zb}, {ze}) after {k} launches", vol, ref_t, ref_w, DIMS)
            assert vol.summary_stats() == (total, 0, total), f"after launch {k}: every segment carries the count {k}"


def _state(cfg, weight, seed=3):
    """A slab state: TSDF random in (-0.9, 0.9), the given weight everywhere."""
    n = DIMS[0] * DIMS[1] * (cfg.z_end - cfg.z_begin)
    t = np.random.default_rng(seed).uniform(-0.9, 0.9, n).astype(np.float32)
    return t, np.full(n, weight, np.float32)


SPECIALS = np.array([2.0 ** -120, -(2.0 ** -140), 0.0, -0.0, np.nan], np.float32)


@pytest.mark.parametrize("zb,ze", SLABS)
def test_zero_distance_and_special_tsdf_values(cuda, oracle, zb, ze):
    """The numerator 0 of diff / trunc: identity pose and a constant depth equal to one slice's camera z (the x and y terms of
    cz are exact zeros under the identity rotation) put diff, and dist, at exactly 0 there, and a few voxels off in the
    slices beside it.  Uniform weights 3 (runs everywhere) and special TSDF values (2^-120, a denormal, +-0, NaN) scattered
    through every third segment make the running mean's numerators tsdf * 3 + 0 tiny, denormal, zero and NaN in that slice.
    All of it must equal the oracle."""
    scene(cuda)
    cfg = config(zb, ze)
    total = segments(cfg)
    t, w = _state(cfg, 3.0, seed=5)
    rng = np.random.default_rng(9)
    seg = t.reshape(-1, 256)
    special = np.arange(len(seg)) % 3 == 1
    for s in np.flatnonzero(special):
        at = rng.choice(256, 12, replace=False)
        seg[s, at] = SPECIALS[rng.integers(0, len(SPECIALS), at.size)]
    assert bool(np.signbit(t[t == 0]).any()) and bool(np.isnan(t).any())
    z_flat = zb + 1                                                # the slice whose dist is exactly 0
    cam_z = np.float32(_S["origin"][2]) + np.float32(z_flat) * np.float32(VS)
    depth = np.full_like(_S["full"], cam_z)
    depth_dev = cuda.from_numpy(depth).cuda()
    pose = synth.identity_pose()
    with volume(cfg) as vol:
        vol.upload(t, w)
        assert vol.summary_stats()[2] == total
        before = t.copy()
        vol.integrate_device(depth_dev.data_ptr(), pose)
        oracle_step(oracle, cfg, pose, depth, t, w)
        per = DIMS[0] * DIMS[1]
        flat = slice((z_flat - zb) * per, (z_flat - zb + 1) * per)
        assert bool(np.all(w == 4.0)), "the frame updates every voxel"
        ordinary = np.isfinite(before[flat]) & (np.abs(before[flat]) > 0.01)
        assert np.array_equal(t[flat][ordinary], (before[flat][ordinary] * np.float32(3.0)) / np.float32(4.0)), \
            "dist is exactly 0 in the chosen slice"
        assert_equals_oracle(vol, t, w, "special numerators")
        assert vol.summary_stats()[2] == total


@pytest.mark.parametrize("zb,ze", SLABS)
def test_wide_truncation_takes_the_compilers_first_division(cuda, oracle, zb, ze):
    """trunc_margin 2^21 is outside what trunc_fast admits: diff / trunc is the compiler's."""
    S = scene(cuda)
    cfg = config(zb, ze, trunc=2097152.0)
    total = segments(cfg)
    t, w = oracle.init_grid(DIMS, zb, ze)
    with volume(cfg) as vol:
        for k in range(3):
            vol.integrate_device(S["full_dev"].data_ptr(), S["poses"][k])
            oracle_step(oracle, cfg, S["poses"][k], S["full"], t, w)
            assert_equals_oracle(vol, t, w, f"trunc 2^21, launch {k + 1}")
        assert bool(np.all(t < 1.0)) and vol.summary_stats() == (total, 0, total)
