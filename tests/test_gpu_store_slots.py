"""Who holds the slots of the shared frame store (csrc/frame_store.h) when: tsdf_store_stats after every call of the paths that
take frame, mask and tile-table slots.  A slot is held by the call that fills it, or by the frames a deferring handle has
collected, and by nothing else: once a call has queued the slot's last reader the handle holds none, and a flush hands back
what was collected.  The counts asserted are conditions that follow from the code on paths that succeed, not measurements.

The images are 120 x 160, a size no other test creates a volume with: the store is this file's own, so the class totals are
exact as well."""
import numpy as np
import pytest

from semantic_slam_amd import capi, synth

pytestmark = pytest.mark.gpu

H, W = 120, 160
K = synth.TUM_K.copy()
K[[0, 2, 4, 5]] *= 0.25                      # the TUM camera at a quarter of its resolution
VS = 0.02
GRID, GRID_NO_FUSE = (64, 16, 8), (37, 20, 12)     # dim_x % 4 != 0: no fused launch, the one-voxel-per-lane kernel
CLASSES = ("frames", "masks", "tables")


def setup(dims, n):
    origin = synth.surf_volume(dims[0], VS, 0.8)
    cfg = capi.make_config(dims, VS, origin, K=K, im_height=H, im_width=W)
    sc = synth.SurfScene(dims, VS, origin, K=K, h=H, w=W)
    poses = [sc.pose(k % 9, 11) for k in range(n)]
    return cfg, origin, [(p, sc.depth(p, quantize=True)) for p in poses]


def held(vol):
    return {name: counts[0] for name, counts in vol.store_stats().items()}


NONE_HELD = dict.fromkeys(CLASSES, 0)


def equal_bits(vol, ref_t, ref_w):
    t, w = vol.download()
    return np.array_equal(w, ref_w) and np.array_equal(t.view(np.uint32), ref_t.view(np.uint32))


@pytest.mark.parametrize("dims", [GRID, GRID_NO_FUSE])
def test_collected_host_frames_hold_their_slots_until_the_flush(cuda, oracle, dims):
    cfg, origin, frames = setup(dims, 12)
    ref_t, ref_w = oracle.init_grid(dims)
    with capi.Volume(cfg) as vol:
        vol.set_deferral(5)
        for k, (pose, depth) in enumerate(frames):
            vol.integrate(depth, pose)
            oracle.integrate(cfg.cam_K, pose, depth, dims, origin, VS, cfg.trunc_margin, ref_t, ref_w)
            assert held(vol) == {"frames": (k + 1) % 5, "masks": 0, "tables": 0}, k     # 1, 2, 3, 4, then the flush: 0
        assert equal_bits(vol, ref_t, ref_w)           # applies the two frames still collected
        assert held(vol) == NONE_HELD
    assert ref_w.max() >= 5


def test_collected_device_and_masked_frames_hold_frame_and_mask_slots(cuda, oracle):
    cfg, origin, frames = setup(GRID, 12)
    mask = np.zeros((H, W), np.uint8)
    mask[20:100, 30:130] = 255
    m_dev = cuda.from_numpy(mask).cuda()
    dev = [cuda.from_numpy(d).cuda() for _, d in frames]
    kinds = "hdmhm" "mmdhh" "dm"                       # host, device-resident, masked device-resident
    ref_t, ref_w = oracle.init_grid(GRID)
    with capi.Volume(cfg) as vol:
        vol.set_deferral(5)
        masked = 0
        for k, (kind, (pose, depth)) in enumerate(zip(kinds, frames)):
            if kind == "h":
                vol.integrate(depth, pose)
            elif kind == "d":
                vol.integrate_device(dev[k].data_ptr(), pose)
            else:
                vol.integrate_masked_device(dev[k].data_ptr(), m_dev.data_ptr(), pose)
            seen = oracle.mask_depth(depth, mask) if kind == "m" else depth
            oracle.integrate(cfg.cam_K, pose, seen, GRID, origin, VS, cfg.trunc_margin, ref_t, ref_w)
            masked = 0 if (k + 1) % 5 == 0 else masked + (kind == "m")
            assert held(vol) == {"frames": (k + 1) % 5, "masks": masked, "tables": 0}, k
        assert equal_bits(vol, ref_t, ref_w)
        assert held(vol) == NONE_HELD
    assert ref_w.max() >= 5


def test_one_kernel_per_call_holds_nothing_between_calls(cuda):
    cfg, origin, frames = setup(GRID, 6)
    raw = [np.round(d * 5000.0).astype(np.uint16) for _, d in frames]
    rgb = np.random.default_rng(5).integers(0, 256, (H, W, 3), dtype=np.uint8)
    with capi.Volume(cfg) as vol:
        vol.set_deferral(0)
        vol.colour_enable()
        for k, (pose, depth) in enumerate(frames):
            vol.integrate(depth, pose)
            assert held(vol) == NONE_HELD, k
            vol.integrate_u16(raw[k], pose)
            assert held(vol) == NONE_HELD, k
            vol.integrate_rgbd(depth, rgb, pose)
            assert held(vol) == NONE_HELD, k
        # a raw frame takes two slots a call and a handle reuses its own once it has its quota of 64: the class stops growing
        totals = []
        for _ in range(2):
            for k in range(200):
                vol.integrate_u16(raw[k % 6], frames[k % 6][0])
            assert held(vol) == NONE_HELD
            totals.append(vol.store_stats()["frames"][2])
        assert totals[0] == totals[1], totals
        vol.sync()


def test_sequence_launches_give_their_table_slot_back(cuda):
    cfg, origin, frames = setup(GRID, 40)
    dev = [cuda.from_numpy(d).cuda() for _, d in frames]
    ptrs, poses = [d.data_ptr() for d in dev], np.stack([p for p, _ in frames])
    lab = cuda.full((H, W), 3, dtype=cuda.uint16, device="cuda")
    score = cuda.full((H, W), 0.75, dtype=cuda.float32, device="cuda")
    with capi.Volume(cfg) as vol:
        vol.set_kernel_variant(8)                      # every fused launch classifies: a table slot each
        vol.labels_enable(0.5)
        vol.integrate_frames_device(ptrs[:3], poses[:3])
        assert held(vol) == NONE_HELD
        assert vol.store_stats()["tables"][1] >= 1     # ... which has gone back by stream order
        vol.integrate_frames_device(ptrs, poses)       # two launches, the second one's pre-pass beside the first
        assert held(vol) == NONE_HELD
        vol.integrate_frames_labels_device(ptrs[:7], [lab.data_ptr()] * 7, [score.data_ptr()] * 7, poses[:7])
        assert held(vol) == NONE_HELD
        vol.sync()


@pytest.mark.parametrize("dims", [GRID, (256, 16, 8)])      # the flat mapping and the row mapping, both by wavefront bricks
def test_masked_classified_one_frame_launch_gives_its_table_slot_back(cuda, oracle, dims):
    cfg, origin, frames = setup(dims, 1)
    pose, depth = frames[0]
    mask = np.zeros((H, W), np.uint8)
    mask[20:100, 30:130] = 255
    d_dev, m_dev = cuda.from_numpy(depth).cuda(), cuda.from_numpy(mask).cuda()
    ref_t, ref_w = oracle.init_grid(dims)
    oracle.integrate(cfg.cam_K, pose, oracle.mask_depth(depth, mask), dims, origin, VS, cfg.trunc_margin, ref_t, ref_w)
    with capi.Volume(cfg) as vol:
        vol.set_kernel_variant(8)
        vol.set_deferral(0)
        vol.integrate_masked_device(d_dev.data_ptr(), m_dev.data_ptr(), pose)
        assert held(vol) == NONE_HELD
        assert vol.store_stats()["tables"][1] == 1
        assert equal_bits(vol, ref_t, ref_w)


@pytest.mark.parametrize("defer,n", [(0, 5), (32, 34)])
def test_group_slabs_hold_nothing_between_calls(cuda, oracle, defer, n):
    cfg, origin, frames = setup(GRID, n)
    ref_t, ref_w = oracle.init_grid(GRID)
    with capi.Group(cfg, [0, 0, 0]) as grp:
        grp.set_deferral(defer)
        for k, (pose, depth) in enumerate(frames):
            grp.integrate(depth, pose)
            oracle.integrate(cfg.cam_K, pose, depth, GRID, origin, VS, cfg.trunc_margin, ref_t, ref_w)
            assert [held(s) for s in grp.slabs] == [NONE_HELD] * 3, k
        t, w = grp.download()
        assert [held(s) for s in grp.slabs] == [NONE_HELD] * 3
    assert np.array_equal(w, ref_w) and np.array_equal(t.view(np.uint32), ref_t.view(np.uint32))
