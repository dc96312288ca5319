"""Sweep order of the one-frame kernel (integrate_tile): successive launches sweep z in alternate directions and keep the
last slices of each sweep in the Infinity Cache (csrc/tsdf_capi.hip, set_sweep).  The order is a performance hint only:
every voxel's update reads its own state, the frame and the pose.  So after any number of launches, in any mix with the
other paths, every TSDF and weight bit equals the reference kernel's replay (tests/whole_volume.py)."""
import numpy as np
import pytest

import whole_volume as wv
from semantic_slam_amd import capi, synth

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not wv.available(), reason="oracle/_ref/libtsdf_ref_hip.so not built")]


def _scene(torch, name, dims, n, vs=0.005):
    """(trunc, origin, cam2base poses [n, 16] (base = identity), device depth frames, host depth frames)."""
    if name == "sband" or name == "sfull":
        origin = synth.sband_volume(dims, vs) if name == "sband" else synth.sfull_volume(dims, vs)
        trunc = synth.SBAND_TRUNC if name == "sband" else None
        pose = synth.sband_pose if name == "sband" else synth.sfull_pose
        poses = np.stack([pose(k) for k in range(n)])
        depths = [synth.sfull_depth()] * n
    else:
        origin = synth.surf_volume(dims[0], vs, 1.0)
        scene = synth.SurfScene(dims, vs, origin)
        poses = np.stack([scene.pose(k, 64) for k in range(n)])
        depths = [scene.depth(p, quantize=True) for p in poses]
        if name == "ssurf_noisy":
            depths = synth.sensor_imperfections(depths, 2.0, 0.05)
        trunc = None
    return trunc, origin, poses, [torch.from_numpy(d).cuda() for d in depths], depths


def _check(torch, what, vol, cfg, dims, poses, dev, n, key):
    ref_t, ref_w = wv.replay(torch, key, cfg.cam_K, dims, cfg.origin, cfg.voxel_size, cfg.trunc_margin, poses[:n], dev[:n])
    wv.assert_volume_equals_reference(torch, f"{what} after {n} launches", vol, ref_t, ref_w, dims)
    wv.drop(key)


# 512^3 (the bench's grid, 1 GiB of state: a window of the last slices of each sweep); slabs with z_begin != 0 whose state
# is smaller than the window (swept cacheable throughout) and larger than it; rows per slice not a multiple of 8 (the
# last workgroup row of every slice is partial).
SHAPES = [((512, 512, 512), 0, 512), ((512, 512, 512), 192, 256), ((512, 512, 512), 100, 420), ((512, 500, 300), 37, 300),
          ((256, 203, 160), 0, 160)]


# the odd shapes run S-band (every voxel updated by every launch)
CASES = [(name, SHAPES[0]) for name in ("ssurf", "ssurf_noisy")] + [("sband", s) for s in SHAPES]


@pytest.mark.parametrize("name,shape", CASES, ids=lambda c: c if isinstance(c, str) else f"{c[0][0]}x{c[0][1]}x{c[0][2]}_z{c[1]}-{c[2]}")
def test_alternating_one_frame_launches_equal_the_reference(cuda, name, shape):
    dims, zb, ze = shape
    trunc, origin, poses, dev, _ = _scene(cuda, name, dims, 7)
    cfg = capi.make_config(dims, 0.005, origin, trunc=trunc, z_begin=zb, z_end=ze)
    with capi.Volume(cfg) as vol:
        vol.set_deferral(0)
        for k in range(7):
            vol.integrate_device(dev[k].data_ptr(), poses[k])
            if k + 1 in (1, 2, 3, 7):
                _check(cuda, f"{name} {dims} z [{zb}, {ze})", vol, cfg, dims, poses, dev, k + 1, f"sweep_{name}_{dims}_{k + 1}")


@pytest.mark.parametrize("dims,zb,ze", [((512, 512, 512), 0, 512), ((512, 500, 96), 5, 96)])
def test_masked_one_frame_launches_unclassified_equal_the_reference(cuda, dims, zb, ze):
    """integrate_tile<2, true> (variant 7: never classified): depth x (mask >= 128) as the reference sees it."""
    trunc, origin, poses, dev, _ = _scene(cuda, "ssurf", dims, 5)
    rng = np.random.default_rng(5)
    masks = [cuda.from_numpy(np.where(rng.random((480, 640)) < 0.7, 255, 0).astype(np.uint8)).cuda() for _ in range(5)]
    masked = [d * (m >= 128).float() for d, m in zip(dev, masks)]
    cfg = capi.make_config(dims, 0.005, origin, trunc=trunc, z_begin=zb, z_end=ze)
    with capi.Volume(cfg) as vol:
        vol.set_kernel_variant(7)
        vol.set_deferral(0)
        for k in range(5):
            vol.integrate_masked_device(dev[k].data_ptr(), masks[k].data_ptr(), poses[k])
            if k + 1 in (1, 2, 5):
                _check(cuda, f"masked {dims} z [{zb}, {ze})", vol, cfg, dims, poses, masked, k + 1, f"sweep_masked_{dims}_{k + 1}")


def test_odd_launch_counts_interleaved_with_the_other_paths(cuda):
    """An odd number of one-frame launches between fused, deferred, reset, upload, colour and label calls: the handle's
    sweep parity lands on every value at every boundary, and the volume still equals the reference's replay."""
    dims = (512, 512, 256)
    _, origin, poses, dev, host = _scene(cuda, "ssurf", dims, 13)
    cfg = capi.make_config(dims, 0.005, origin)
    rgb = cuda.zeros((480, 640, 3), dtype=cuda.uint8).cuda() + 7
    lab = cuda.ones((480, 640), dtype=cuda.int16).cuda().view(cuda.uint16) if hasattr(cuda, "uint16") else None
    with capi.Volume(cfg) as vol:
        vol.colour_enable()
        vol.labels_enable(0.5)
        one = lambda k: (vol.set_deferral(0), vol.integrate_device(dev[k].data_ptr(), poses[k]))
        for k in range(3):
            one(k)
        vol.integrate_colour_device(dev[2].data_ptr(), rgb.data_ptr(), poses[2])
        vol.integrate_frames_device([d.data_ptr() for d in dev[3:6]], poses[3:6])          # fused
        if lab is not None:
            score = cuda.full((480, 640), 0.9, dtype=cuda.float32).cuda()
            vol.integrate_labels_device(dev[5].data_ptr(), lab.data_ptr(), score.data_ptr(), poses[5])
        vol.set_deferral(32)
        for k in (6, 7):                                                                     # deferred host frames
            vol.integrate(host[k], poses[k])
        one(8)
        _check(cuda, "interleaved", vol, cfg, dims, poses, dev, 9, "sweep_mix_9")
        t, w = vol.download()
        vol.upload(t, w)                                                                     # summary rebuilt from the arrays
        one(9)
        _check(cuda, "after upload", vol, cfg, dims, poses, dev, 10, "sweep_mix_10")
        vol.reset()
        for k in range(3):
            one(k)
        _check(cuda, "after reset", vol, cfg, dims, poses, dev, 3, "sweep_mix_3")


def test_summary_refresh_and_free_space_under_alternating_sweeps(cuda):
    """The free-space summary the kernel keeps while sweeping both ways is what a rebuild from the arrays gives: a volume
    whose summary is refreshed between launches ends bit-identical to one that never is; S-full stays exactly 1."""
    dims = (512, 512, 512)
    _, origin, poses, dev, _ = _scene(cuda, "ssurf", dims, 5)
    cfg = capi.make_config(dims, 0.005, origin)
    out = []
    for refresh in (False, True):
        with capi.Volume(cfg) as vol:
            vol.set_deferral(0)
            for k in range(5):
                vol.integrate_device(dev[k].data_ptr(), poses[k])
                if refresh:
                    capi.check(vol.lib.tsdf_refresh_summary(vol._h), "tsdf_refresh_summary")
            out.append(wv.product_arrays(cuda, vol))
    wv.assert_same_bits(cuda, "summary refreshed vs kept", out[1][0], out[1][1], out[0][0], out[0][1], dims)
    del out
    _, origin, poses, dev, _ = _scene(cuda, "sfull", dims, 5)
    cfg = capi.make_config(dims, 0.005, origin)
    with capi.Volume(cfg) as vol:
        vol.set_deferral(0)
        for k in range(5):
            vol.integrate_device(dev[k].data_ptr(), poses[k])
        t, w = wv.product_arrays(cuda, vol)
    assert bool((t == 1.0).all()) and bool((w == 5.0).all())


def test_graph_probe_volume_matches(cuda):
    """tsdf_probe_graph_replay captures one-frame launches into a graph and replays them: the parity the capture baked in
    repeats on every replay, which changes the order only."""
    dims = (512, 512, 128)
    trunc, origin, poses, dev, _ = _scene(cuda, "sband", dims, 6)
    cfg = capi.make_config(dims, 0.005, origin, trunc=trunc)
    with capi.Volume(cfg) as a, capi.Volume(cfg) as b:
        a.probe_graph_replay(dev[0].data_ptr(), poses, iters=3)
        ta, wa = a.download()
        b.probe_graph_replay(dev[0].data_ptr(), poses, iters=3)
        tb, wb = b.download()
    assert wa.max() > 0
    assert np.array_equal(wa, wb) and np.array_equal(ta.view(np.uint32), tb.view(np.uint32))
