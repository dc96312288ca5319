"""Weight runs of the one-frame kernel (integrate_tile; csrc/host_derive.h, "the summary word"): while a 256-voxel segment's
word says "every weight is the count c" the kernel takes the weights from the word instead of loading them.  Whatever the
word says, every TSDF and weight bit must equal the reference kernel's replay (tests/whole_volume.py) or, for uploaded
states, the CPU oracle; and tsdf_summary_stats must show that the shortcut was taken (or dropped) where the rule says so.

Shapes: 512 x 9 x 6 -- two segments per row, an odd dim_y so that the last pair of rows a lane owns is partial -- whole and
as the slab z [2, 5).  Every comparison is bit for bit."""
import numpy as np
import pytest

import fuse_spec as fs
import whole_volume as wv
from semantic_slam_amd import capi, synth

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not wv.available(), reason="oracle/_ref/libtsdf_ref_hip.so not built")]

DIMS, VS = (512, 9, 6), 0.005
SLABS = [(0, 6), (2, 5)]
N = 8
_S = {}


def scene(torch):
    """S-band and S-full over DIMS, once per session: origin, poses, the constant depth frame, a frame with a rectangle of
    zero depth (segment 0 of the upper voxel rows sees nothing, segment 1 of them is partly updated, the lower rows wholly),
    masks of random blocks; on the host and on the device."""
    if not _S:
        full = synth.sfull_depth()
        broken = full.copy()
        broken[:246, :330] = 0.0
        rng = np.random.default_rng(11)
        masks = [np.repeat(np.repeat(np.where(rng.random((240, 10)) < 0.7, 255, 0).astype(np.uint8), 2, axis=0), 64, axis=1) for _ in range(3)]
        _S.update(origin=synth.sband_volume(DIMS, VS), band_poses=np.stack([synth.sband_pose(k) for k in range(N)]),
                  full_poses=np.stack([synth.sfull_pose(k) for k in range(N)]), full=full, broken=broken, masks=masks,
                  full_dev=torch.from_numpy(full).cuda(), broken_dev=torch.from_numpy(broken).cuda(),
                  masks_dev=[torch.from_numpy(m).cuda() for m in masks])
        assert np.array_equal(_S["origin"], synth.sfull_volume(DIMS, VS))
    return _S


def config(name, zb=0, ze=DIMS[2]):
    S = _S
    return capi.make_config(DIMS, VS, S["origin"], trunc=synth.SBAND_TRUNC if name == "sband" else None, z_begin=zb, z_end=ze)


def reference(torch, key, cfg, poses, frames):
    """The reference kernel's replay of the frames over the whole grid (cached under the key, shared, never changed)."""
    return wv.replay(torch, "runs_" + key, cfg.cam_K, DIMS, cfg.origin, cfg.voxel_size, cfg.trunc_margin, list(poses), list(frames))


def segments(cfg):
    return 2 * DIMS[1] * (cfg.z_end - cfg.z_begin)


def seg_view(torch, w, cfg):
    """[segments, 256] view of the slab's part of a whole-grid weight tensor."""
    per = DIMS[0] * DIMS[1]
    return w[cfg.z_begin * per:cfg.z_end * per].reshape(-1, 256)


def runs_kept(torch, cfg, weights):
    """How many segments still carry a run after the launches whose whole-grid weights are given in order (from a fresh
    volume): those that every launch updated wholly or not at all, by the rule -- counted from the reference's weights."""
    keep, prev = None, None
    for w in weights:
        s = seg_view(torch, w, cfg)
        d = s if prev is None else s - prev
        uniform = d.min(dim=1).values == d.max(dim=1).values
        keep = uniform if keep is None else keep & uniform
        prev = s
    return int(keep.sum())


def one(vol, depth_dev, pose):
    vol.integrate_device(depth_dev.data_ptr(), pose)


def volume(cfg, variant=None):
    vol = capi.Volume(cfg)
    vol.set_deferral(0)
    if variant is not None:
        vol.set_kernel_variant(variant)
    return vol


@pytest.mark.parametrize("zb,ze", SLABS)
def test_sband_counts_up_in_every_segment(cuda, zb, ze):
    S = scene(cuda)
    cfg = config("sband", zb, ze)
    total = segments(cfg)
    with volume(cfg) as vol:
        assert vol.summary_stats() == (total, total, total), "a fresh volume: TSDF 1 and the count 0 everywhere"
        for k in range(1, 6):
            one(vol, S["full_dev"], S["band_poses"][k - 1])
            ref_t, ref_w = reference(cuda, f"sband_{k}", cfg, S["band_poses"][:k], [S["full_dev"]] * k)
            assert bool((ref_w == float(k)).all()) and bool((ref_t < 1.0).all()), "S-band updates every voxel inside the band"
            wv.assert_volume_equals_reference(cuda, f"S-band z [{zb}, {ze}) after {k} launches", vol, ref_t, ref_w, DIMS)
            assert vol.summary_stats() == (total, 0, total), f"after launch {k}: no segment is all ones, every segment carries the count"


@pytest.mark.parametrize("zb,ze", SLABS)
def test_a_partly_updated_segment_ends_its_run(cuda, zb, ze):
    S = scene(cuda)
    cfg = config("sband", zb, ze)
    total = segments(cfg)
    poses = S["band_poses"]
    frames = [S["broken_dev"], S["full_dev"], S["full_dev"]]
    with volume(cfg) as vol:
        weights = []
        for k in range(1, 4):
            one(vol, frames[k - 1], poses[k - 1])
            ref_t, ref_w = reference(cuda, f"broken_{k}", cfg, poses[:k], frames[:k])
            weights.append(ref_w)
            wv.assert_volume_equals_reference(cuda, f"broken run z [{zb}, {ze}) after {k} launches", vol, ref_t, ref_w, DIMS)
            if k == 1:       # the frame is what it is meant to be: segments untouched, partly and wholly updated
                s = seg_view(cuda, ref_w, cfg)
                lo, hi = s.min(dim=1).values, s.max(dim=1).values
                untouched, whole, partly = int((hi == 0).sum()), int((lo == 1).sum()), int((lo != hi).sum())
                assert untouched > 0 and whole > 0 and partly > 0 and untouched + whole + partly == total
                kept = total - partly
            assert runs_kept(cuda, cfg, weights) == kept
            assert vol.summary_stats()[2] == kept, f"after launch {k}: the partly updated segments lost their run, the others kept it"


@pytest.mark.parametrize("zb,ze", SLABS)
def test_free_space_keeps_ones_and_counts(cuda, zb, ze):
    S = scene(cuda)
    cfg = config("sfull", zb, ze)
    total = segments(cfg)
    with volume(cfg) as vol:
        for k in range(1, 4):
            one(vol, S["full_dev"], S["full_poses"][k - 1])
            ref_t, ref_w = reference(cuda, f"sfull_{k}", cfg, S["full_poses"][:k], [S["full_dev"]] * k)
            wv.assert_volume_equals_reference(cuda, f"S-full z [{zb}, {ze}) after {k} launches", vol, ref_t, ref_w, DIMS)
            assert vol.summary_stats() == (total, total, total)
        t, w = wv.product_arrays(cuda, vol)
        assert bool((t.view(cuda.int32) == 0x3f800000).all()) and bool((w == 3.0).all())


@pytest.mark.parametrize("zb,ze", SLABS)
def test_masked_one_frame_launches(cuda, zb, ze):
    """integrate_tile<2, true> (variant 7: never classified) against the reference on depth x mask."""
    S = scene(cuda)
    cfg = config("sband", zb, ze)
    total = segments(cfg)
    masked = [S["full_dev"] * (m >= 128).float() for m in S["masks_dev"]]
    with volume(cfg, 7) as vol:
        weights = []
        for k in range(1, 4):
            vol.integrate_masked_device(S["full_dev"].data_ptr(), S["masks_dev"][k - 1].data_ptr(), S["band_poses"][k - 1])
            ref_t, ref_w = reference(cuda, f"masked_{k}", cfg, S["band_poses"][:k], masked[:k])
            weights.append(ref_w)
            wv.assert_volume_equals_reference(cuda, f"masked z [{zb}, {ze}) after {k} launches", vol, ref_t, ref_w, DIMS)
            kept = runs_kept(cuda, cfg, weights)
            if k == 1:
                assert 0 < kept < total, "the masks must break some runs and leave some"
            assert vol.summary_stats()[2] == kept


# ------------------------------------------------------------------------------------------------------------------------
# hand-overs: the other writers of weights, each followed by a one-frame launch
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("zb,ze", SLABS)
def test_fused_launch_forgets_the_runs(cuda, zb, ze):
    S = scene(cuda)
    cfg = config("sband", zb, ze)
    total = segments(cfg)
    poses, d = S["band_poses"], S["full_dev"]
    with volume(cfg) as vol:
        for k in range(2):
            one(vol, d, poses[k])
        assert vol.summary_stats()[2] == total
        vol.integrate_frames_device([d.data_ptr()] * 3, poses[2:5])
        assert vol.summary_stats()[2] == 0, "after a fused launch bit 2 is clear everywhere"
        ref_t, ref_w = reference(cuda, "sband_5", cfg, poses[:5], [d] * 5)
        wv.assert_volume_equals_reference(cuda, "after the fused launch", vol, ref_t, ref_w, DIMS)
        one(vol, d, poses[5])
        ref_t, ref_w = reference(cuda, "sband_6", cfg, poses[:6], [d] * 6)
        wv.assert_volume_equals_reference(cuda, "one-frame launch after the fused one", vol, ref_t, ref_w, DIMS)
        assert vol.summary_stats()[2] == 0, "no launch starts a run"


@pytest.mark.parametrize("zb,ze", SLABS)
def test_masked_brick_launch_forgets_the_runs(cuda, zb, ze):
    S = scene(cuda)
    cfg = config("sband", zb, ze)
    total = segments(cfg)
    poses, d, m = S["band_poses"], S["full_dev"], S["masks_dev"][0]
    frames = [d, d, d * (m >= 128).float(), d]
    with volume(cfg) as vol:
        for k in range(2):
            one(vol, d, poses[k])
        assert vol.summary_stats()[2] == total
        vol.set_kernel_variant(8)                     # always classified: wavefront bricks
        vol.integrate_masked_device(d.data_ptr(), m.data_ptr(), poses[2])
        assert vol.summary_stats()[2] == 0
        vol.set_kernel_variant(0)
        one(vol, d, poses[3])
        ref_t, ref_w = reference(cuda, "bricks_4", cfg, poses[:4], frames)
        wv.assert_volume_equals_reference(cuda, "one-frame launch after masked bricks", vol, ref_t, ref_w, DIMS)


@pytest.mark.parametrize("zb,ze", SLABS)
def test_scalar_kernel_and_reset(cuda, zb, ze):
    S = scene(cuda)
    cfg = config("sband", zb, ze)
    total = segments(cfg)
    poses, d = S["band_poses"], S["full_dev"]
    with volume(cfg) as vol:
        for k in range(2):
            one(vol, d, poses[k])
        vol.set_kernel_variant(1)                     # the scalar kernel keeps no summary at all
        one(vol, d, poses[2])
        assert vol.summary_stats() == (total, 0, 0)
        vol.set_kernel_variant(0)
        one(vol, d, poses[3])
        ref_t, ref_w = reference(cuda, "sband_4", cfg, poses[:4], [d] * 4)
        wv.assert_volume_equals_reference(cuda, "one-frame launch after the scalar kernel", vol, ref_t, ref_w, DIMS)
        assert vol.summary_stats() == (total, 0, 0)
        vol.reset()
        assert vol.summary_stats() == (total, total, total)
        one(vol, d, poses[0])
        ref_t, ref_w = reference(cuda, "sband_1", cfg, poses[:1], [d])
        wv.assert_volume_equals_reference(cuda, "one-frame launch after reset", vol, ref_t, ref_w, DIMS)
        assert vol.summary_stats() == (total, 0, total)


def _state(cfg, weight, seed=3):
    """A slab state: TSDF random in (-0.9, 0.9) with a quarter of the segments all ones, the given weight everywhere."""
    n = DIMS[0] * DIMS[1] * (cfg.z_end - cfg.z_begin)
    rng = np.random.default_rng(seed)
    t = rng.uniform(-0.9, 0.9, n).astype(np.float32).reshape(-1, 256)
    t[rng.random(len(t)) < 0.25] = 1.0
    return t.ravel().copy(), np.full(n, weight, np.float32)


UPLOADS = [("uniform_3", 3.0, "all"), ("uniform_2.5", 2.5, "none"), ("minus_zero", -0.0, "none"), ("one_voxel_differs", 3.0, "all_but_one")]


@pytest.mark.parametrize("zb,ze", SLABS)
@pytest.mark.parametrize("name,weight,expect", UPLOADS, ids=[u[0] for u in UPLOADS])
def test_upload_sets_the_run_only_for_a_uniform_count(cuda, oracle, name, weight, expect, zb, ze):
    S = scene(cuda)
    cfg = config("sband", zb, ze)
    total = segments(cfg)
    t, w = _state(cfg, weight)
    if expect == "all_but_one":
        w[256 * 7 + 255] = 4.0
    assert name != "minus_zero" or bool(np.all(w.view(np.uint32) == 0x80000000))
    with volume(cfg) as vol:
        one(vol, S["full_dev"], S["band_poses"][0])           # the words hold runs of another state
        vol.upload(t, w)
        want_runs = {"all": total, "none": 0, "all_but_one": total - 1}[expect]
        assert vol.summary_stats()[2] == want_runs
        for k in (1, 2):
            one(vol, S["full_dev"], S["band_poses"][k])
            oracle.integrate(cfg.cam_K, oracle.cam2base(synth.identity_pose(), S["band_poses"][k]), S["full"], DIMS, S["origin"], VS,
                             cfg.trunc_margin, t, w, z_begin=zb, z_end=ze)
            got_t, got_w = vol.download()
            assert np.array_equal(got_w.view(np.uint32), w.view(np.uint32)), f"{name}: weights differ from the oracle after launch {k}"
            assert np.array_equal(got_t.view(np.uint32), t.view(np.uint32)), f"{name}: TSDF differs from the oracle after launch {k}"
        assert vol.summary_stats()[2] == want_runs, "S-band updates whole segments: the runs that were there go on"


def test_merge_into_the_handle_rebuilds_the_words(cuda, oracle):
    """tsdf_fuse_volume with write: the words are rebuilt from the arrays, and the next one-frame launch computes from them."""
    S = scene(cuda)
    cfg = config("sband")
    total = segments(cfg)
    sdims = (40, 8, 6)
    scfg = capi.make_config(sdims, VS, np.array([-0.1, -0.02, 3.2], np.float32), trunc=synth.SBAND_TRUNC)
    rng = np.random.default_rng(5)
    st = rng.uniform(-0.9, 0.9, int(np.prod(sdims))).astype(np.float32)
    sw = rng.choice(np.array([1.0, 2.0, 3.0], np.float32), st.size)
    poses, d = S["band_poses"], S["full_dev"]
    ref_t, ref_w = reference(cuda, "sband_2", cfg, poses[:2], [d] * 2)
    want_t, want_w, want_counts = fs.fuse(ref_t.cpu().numpy(), ref_w.cpu().numpy(), fs.grid_of(cfg), st, sw, fs.grid_of(scfg))
    assert 0 < int((want_w != 2.0).sum()) < want_w.size, "the merge must change some weights and leave others"
    oracle.integrate(cfg.cam_K, oracle.cam2base(synth.identity_pose(), poses[2]), S["full"], DIMS, S["origin"], VS, cfg.trunc_margin,
                     want_t, want_w)
    with volume(cfg) as vol, capi.Volume(scfg) as src:
        for k in range(2):
            one(vol, d, poses[k])
        src.upload(st, sw)
        assert vol.fuse_from(src) == want_counts
        assert 0 < vol.summary_stats()[2] < total
        one(vol, d, poses[2])
        got_t, got_w = vol.download()
    assert np.array_equal(got_w.view(np.uint32), want_w.view(np.uint32)), "weights after merge + one-frame launch"
    assert np.array_equal(got_t.view(np.uint32), want_t.view(np.uint32)), "TSDF after merge + one-frame launch"


@pytest.mark.parametrize("zb,ze", SLABS)
def test_count_limit(cuda, oracle, zb, ze):
    """Weight 2^24 - 2 everywhere, three S-band launches: 2^24 - 1, 2^24, 2^24, as float addition gives; the run ends once
    the count would pass 2^24 - 1."""
    S = scene(cuda)
    cfg = config("sband", zb, ze)
    total = segments(cfg)
    t, w = _state(cfg, 16777214.0)
    with volume(cfg) as vol:
        vol.upload(t, w)
        assert vol.summary_stats()[2] == total
        for k, (weight, runs) in enumerate([(16777215.0, total), (16777216.0, 0), (16777216.0, 0)]):
            one(vol, S["full_dev"], S["band_poses"][k])
            oracle.integrate(cfg.cam_K, oracle.cam2base(synth.identity_pose(), S["band_poses"][k]), S["full"], DIMS, S["origin"], VS,
                             cfg.trunc_margin, t, w, z_begin=zb, z_end=ze)
            assert bool(np.all(w == np.float32(weight)))
            got_t, got_w = vol.download()
            assert np.array_equal(got_w.view(np.uint32), w.view(np.uint32)), f"weights after launch {k + 1}"
            assert np.array_equal(got_t.view(np.uint32), t.view(np.uint32)), f"TSDF after launch {k + 1}"
            assert vol.summary_stats()[2] == runs, f"runs after launch {k + 1}"
