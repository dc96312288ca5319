"""Handles give back what they take: a volume, a batch and a group are created, driven through every entry point that
allocates on first use (labels, colour, the rgb ring, the frame store's ring and slots, the claims block and side streams of
a pipelined sequence, extraction lists, raycast buffers, the batch's pools and ray block, the group's pool and halo) and
destroyed, cycle after cycle.  Device memory must come back to where it was, and each cycle's store -- destroyed with its
last handle and created afresh -- must hand out slots that integrate correctly."""
import numpy as np
import pytest

from semantic_slam_amd import capi, synth

pytestmark = pytest.mark.gpu

MIB = 1 << 20


def test_create_drive_destroy_releases_device_memory(cuda, oracle, tmp_path):
    dims, vs = (200, 200, 200), 0.004
    origin = synth.surf_volume(dims[0], vs, 0.8)
    cfg = capi.make_config(dims, vs, origin)
    scene = synth.SurfScene(dims, vs, origin)
    poses = [scene.pose(k % 9, 9) for k in range(40)]
    depths = [scene.depth(p, quantize=True) for p in poses]
    h, w = cfg.im_height, cfg.im_width
    rng = np.random.default_rng(5)
    rgb = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    raw_u16 = np.round(depths[1] * 5000.0).astype(np.uint16)
    ref_t, ref_w = oracle.init_grid(dims)
    for p, d in zip(poses[:3], depths[:3]):
        oracle.integrate(cfg.cam_K, p, d, dims, origin, vs, cfg.trunc_margin, ref_t, ref_w)
    assert ref_w.sum() > 0

    member_dims = [(64, 64, 64), (96, 48, 32), (64, 32, 48)]
    member_cfgs = [capi.make_config(d, 0.008, np.array([-0.3 + 0.1 * i, -0.2, 0.8], np.float32), vol_id=i)
                   for i, d in enumerate(member_dims)]
    g_dims, g_vs = (128, 96, 64), 0.008
    g_origin = synth.surf_volume(g_dims[0], g_vs, 0.8)
    g_cfg = capi.make_config(g_dims, g_vs, g_origin)
    g_scene = synth.SurfScene(g_dims, g_vs, g_origin)
    g_frames = [(g_scene.pose(k, 6), g_scene.depth(g_scene.pose(k, 6), quantize=True)) for k in range(6)]

    # every torch buffer exists before the first cycle, so the caching allocator does not move the measurement
    d_dev = [cuda.from_numpy(d).cuda() for d in depths]
    mask_dev = cuda.zeros((h, w), dtype=cuda.uint8).cuda()
    mask_dev[100:380, 120:520] = 255
    ray_depth = cuda.empty((h, w), dtype=cuda.float32, device="cuda")
    ray_normal = cuda.empty((h, w, 3), dtype=cuda.float32, device="cuda")
    ray_member = cuda.empty((h, w), dtype=cuda.int32, device="cuda")
    cuda.cuda.synchronize()

    def cycle():
        with capi.Volume(cfg) as vol:
            for p, d in zip(poses[:3], depths[:3]):
                vol.integrate(d, p)                          # host frames: the store's pinned ring and frame slots
            t, wt = vol.download()
            assert np.array_equal(wt, ref_w) and np.array_equal(t.view(np.uint32), ref_t.view(np.uint32))
            vol.labels_enable(0.5)
            vol.colour_enable()
            vol.integrate_rgbd(depths[0], rgb, poses[0])
            vol.integrate_u16(raw_u16, poses[1])
            vol.integrate_frames_device([x.data_ptr() for x in d_dev], np.stack(poses))   # 32 + 8: pipelined
            assert len(vol.extract_surface()) > 100
            assert len(vol.extract_mesh()) > 0
            vol.raycast(poses[0], labels=True, colour=True)
            vol.save_ply(str(tmp_path / "lifecycle.ply"))
        with capi.Batch(member_cfgs) as batch:
            for k in range(3):
                batch.integrate_device(d_dev[k].data_ptr(), [mask_dev.data_ptr(), None, mask_dev.data_ptr()], poses[k])
            batch.raycast_device(poses[0], ray_depth.data_ptr(), ray_normal.data_ptr(), ray_member.data_ptr())
            batch.sync()
        with capi.Group(g_cfg, [0, 0]) as grp:
            grp.integrate_frames([d for _, d in g_frames], np.stack([p for p, _ in g_frames]))
            assert len(grp.extract_mesh()) > 0
        cuda.cuda.synchronize()
        return cuda.cuda.mem_get_info()[0]

    cycle()                                                  # warm-up: the runtime's own one-off allocations
    free = [cycle() for _ in range(3)]
    assert abs(free[2] - free[0]) <= 4 * MIB, f"free device memory after cycles 1..3: {[f // MIB for f in free]} MiB"
