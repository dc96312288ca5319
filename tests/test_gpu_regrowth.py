"""Buffers that grow on demand and staging rings that wrap, on ONE handle (csrc/hip_owned.h: Growable, StageRing): each call
is held, bit for bit, to a path that does not go through the buffer under test.

  * the output list (tsdf_raycast's host images, then tsdf_extract_surface) over renders of 32 x 24, 96 x 64 and 32 x 24, against
    tsdf_raycast_device into the caller's buffers and the extraction of a handle that never rendered;
  * the tracking scratch block over the same sizes, against fresh handles asked once;
  * a batch's association block over k = 1, 3, 1 masks, against tsdf_associate_count / _assign on the batch's own render;
  * a segmenter's count block over K = 1, 4, 1 masks, against tests/segment_spec.py;
  * 2 * 3 + 1 frames through the colour ring of tsdf_integrate_rgbd and through a batch's ring of parameter blocks, against the
    device-resident entry points on other handles.

All on 32^3 volumes of 8 mm voxels fused from four frames of synth.SurfScene."""
import numpy as np
import pytest

import segment_spec as ss
from semantic_slam_amd import capi, synth

pytestmark = pytest.mark.gpu

f32 = np.float32
DIMS, VS = (32, 32, 32), 0.008
ORIGIN = synth.surf_volume(32, VS, 0.8)
SIZES = [(24, 32), (64, 96), (24, 32)]        # rows x columns: the middle one needs every block regrown, the last one none
N_RING = 2 * 3 + 1                            # kStageSlots = 3: every slot refilled, the first one twice


def camera(hw, zoom=3.0):
    """TUM intrinsics scaled from 480 x 640 to hw, the focal lengths `zoom` times longer: the 0.256 m volume, a quarter of the
    TUM image's width from the orbit, then fills most of a small image."""
    K = np.array(synth.TUM_K, np.float64)
    K[[0, 2]] *= hw[1] / 640.0
    K[[4, 5]] *= hw[0] / 480.0
    K[[0, 4]] *= zoom
    return K.astype(f32)


@pytest.fixture(scope="module")
def frames():
    """(scene, poses, depths): seven 640 x 480 frames of the orbit; the first four are what `fused` holds."""
    scene = synth.SurfScene(DIMS, VS, ORIGIN)
    poses = [scene.pose(k, n=8) for k in range(N_RING)]
    return scene, poses, [scene.depth(c, quantize=True) for c in poses]


@pytest.fixture(scope="module")
def fused(cuda, frames):
    """(tsdf, weight) of the volume after four frames."""
    _, poses, depths = frames
    with capi.Volume(capi.make_config(DIMS, VS, ORIGIN)) as vol:
        for c2w, d in zip(poses[:4], depths[:4]):
            vol.integrate(d, c2w)
        t, w = vol.download()
    assert w.sum() > 1000
    return t, w


def volume_with(state, **cfg):
    vol = capi.Volume(capi.make_config(DIMS, VS, ORIGIN, **cfg))
    vol.upload(*state)
    return vol


def same(got, want, what):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.tobytes() == want.tobytes(), f"{what}: differs"


def rgb_image(k):
    vv, uu = np.mgrid[0:480, 0:640]
    return np.stack([(uu * 3 + 50 * k) % 256, (vv * 2 + 70 * k) % 256, (uu + 2 * vv + 31 * k) % 256], axis=-1).astype(np.uint8)


def test_output_list_regrows_between_raycasts(cuda, frames, fused):
    scene, poses, depths = frames
    cfg = capi.make_config(DIMS, VS, ORIGIN)
    rng = np.random.default_rng(7)
    with capi.Volume(cfg) as vol:
        vol.labels_enable(0.5)
        vol.colour_enable()
        for k, (c2w, d) in enumerate(zip(poses[:4], depths[:4])):
            d_dev = cuda.from_numpy(d).cuda()
            lab = cuda.from_numpy(rng.integers(1, 50, (480, 640)).astype(np.int16)).cuda()
            sc = cuda.from_numpy(rng.uniform(0.3, 1.0, (480, 640)).astype(f32)).cuda()
            rgb = cuda.from_numpy(rgb_image(k)).cuda()
            vol.integrate_device(d_dev.data_ptr(), c2w)
            vol.integrate_colour_device(d_dev.data_ptr(), rgb.data_ptr(), c2w)
            vol.integrate_labels_device(d_dev.data_ptr(), lab.data_ptr(), sc.data_ptr(), c2w)
            vol.sync()
        same(vol.download()[1], fused[1], "weights of the fused volume")
        # the surface list of this volume (300 KB, more than either render needs) from another handle, so that the list buffer
        # of the handle under test starts empty: 17 KB, regrown to 135 KB, kept, regrown for the extraction
        with volume_with(fused) as other:
            before = other.extract_surface()
        assert len(before) > 20000
        view = scene.pose(1, n=8)
        for i, hw in enumerate(SIZES):
            p = capi.raycast_params_default(cfg)
            p.cam_K[:] = [float(x) for x in camera(hw)]
            p.im_height, p.im_width = hw
            got = vol.raycast(view, params=p, normals=True, labels=True, colour=True)
            bufs = {"depth": cuda.full(hw, -7.0, dtype=cuda.float32, device="cuda"),
                    "normal": cuda.full(hw + (3,), -7.0, dtype=cuda.float32, device="cuda"),
                    "label": cuda.full(hw, -7, dtype=cuda.int16, device="cuda"),
                    "colour": cuda.full(hw, -7, dtype=cuda.int32, device="cuda")}
            vol.raycast_device(view, bufs["depth"].data_ptr(), bufs["normal"].data_ptr(), bufs["label"].data_ptr(),
                               bufs["colour"].data_ptr(), params=p)
            vol.sync()
            assert np.count_nonzero(got["depth"]) > hw[0] * hw[1] // 8 and np.count_nonzero(got["colour"]) > 0
            for name, buf in bufs.items():
                same(got[name].view(np.uint8), buf.cpu().numpy().view(np.uint8), f"render {i} ({hw}) {name}")
        same(vol.extract_surface(), before, "the surface list after the renders")
        same(vol.extract_surface(), before, "the surface list again")


def test_track_scratch_regrows_between_sizes(cuda, frames, fused):
    scene, poses, _ = frames
    cfg = capi.make_config(DIMS, VS, ORIGIN)
    ref, cur = scene.pose(1, n=8), scene.pose(3, n=16)            # 10.6 and 13.9 degrees of yaw

    def ask(vol, hw):
        p = capi.track_params_default(cfg)
        p.ray.cam_K[:] = [float(x) for x in camera(hw)]
        p.ray.im_height, p.ray.im_width = hw
        live = synth.SurfScene(DIMS, VS, ORIGIN, K=camera(hw), h=hw[0], w=hw[1]).depth(cur, quantize=True)
        d_dev = cuda.from_numpy(live).cuda()
        A, b, r2, n = vol.track_system(d_dev.data_ptr(), ref, cur, level=0, params=p)
        return np.concatenate([A[np.triu_indices(6)], b, [r2, n]])

    with volume_with(fused) as vol:
        for i, hw in enumerate(SIZES):
            got = ask(vol, hw)
            with volume_with(fused) as fresh:
                want = ask(fresh, hw)
            assert want[28] > 20, f"{hw}: {want[28]} pairs"
            same(got, want, f"system {i} ({hw})")


def two_members():
    return [capi.make_config(DIMS, VS, ORIGIN, vol_id=0),
            capi.make_config(DIMS, VS, ORIGIN + np.array([0.10, 0.02, 0.04], f32), vol_id=1)]


def test_association_block_regrows_with_the_mask_count(cuda, frames):
    scene, poses, depths = frames
    cfgs = two_members()
    view = scene.pose(5, n=8)
    live = cuda.from_numpy(scene.depth(view, quantize=True)).cuda()
    masks = np.zeros((3, 480, 640), np.uint8)
    masks[0, 100:400, 150:420] = 255
    masks[1, 60:300, 330:600] = 255
    masks[2, 200:480, 0:640] = 200
    m_dev = cuda.from_numpy(masks).cuda()
    with capi.Batch(cfgs) as batch:
        for c2w, d in zip(poses[:4], depths[:4]):
            d_dev = cuda.from_numpy(d).cuda()
            batch.integrate_device(d_dev.data_ptr(), None, c2w)
            batch.sync()
        p = capi.associate_params_default(cfgs[0])
        p.min_pixels, p.min_iou = 1, 0.0
        rdepth = cuda.full((480, 640), -7.0, dtype=cuda.float32, device="cuda")
        member = cuda.full((480, 640), -7, dtype=cuda.int32, device="cuda")
        batch.raycast_device(view, rdepth.data_ptr(), None, member.data_ptr(), params=p.ray)
        batch.sync()
        assert set(np.unique(member.cpu().numpy())) >= {0, 1}
        for i, k in enumerate((1, 3, 1)):
            got = batch.associate(view, live.data_ptr(), m_dev.data_ptr(), k, params=p)
            counts = capi.associate_count(p, member.data_ptr(), rdepth.data_ptr(), 2, live.data_ptr(), m_dev.data_ptr(), k)[0]
            assign, iou = capi.associate_assign(p, counts, k, 2)
            assert got["overlap"][..., 0].sum() > 0
            same(got["counts"], counts, f"call {i} (k = {k}) counts")
            same(got["assign"], assign, f"call {i} (k = {k}) assignment")
            same(got["iou"], iou, f"call {i} (k = {k}) IoU")
            assert (assign >= 0).any()


def test_segmenter_count_block_regrows_with_the_mask_count(cuda):
    hw, C = (24, 32), 6
    rng = np.random.default_rng(3)
    cluster = rng.integers(-1, C + 2, hw).astype(np.int32)           # labels outside 1..C count as none
    cluster[4:14, 6:20] = 2
    masks = np.zeros((4,) + hw, np.uint8)
    masks[0, 2:16, 4:24] = 255
    masks[1, 10:24, 0:32] = 128
    masks[2, 0:8, 0:10] = 127
    masks[3] = rng.choice(np.array([0, 127, 128, 255], np.uint8), hw)
    cfg = capi.default_config(*hw)
    cfg.cam_K[:] = [float(x) for x in camera(hw)]
    p = capi.segment_params_default(cfg)
    p.inset, p.overlap = 1, 0.3
    d_cl = cuda.from_numpy(cluster).cuda()
    with capi.Segmenter(*hw) as seg:
        for i, K in enumerate((1, 4, 1)):
            d_m = cuda.from_numpy(masks[:K].copy()).cuda()
            d_out = cuda.full((K,) + hw, 77, dtype=cuda.uint8, device="cuda")
            size, inside = seg.refine_masks(p, d_cl.data_ptr(), C, d_m.data_ptr(), K, d_out.data_ptr())
            want_out, want_counts = ss.refine(cluster, C, masks[:K], ss.from_ctypes(p))
            cuda.cuda.synchronize()
            same(np.concatenate([size, inside.ravel()]), want_counts, f"call {i} (K = {K}) counts")
            same(d_out.cpu().numpy(), want_out, f"call {i} (K = {K}) refined masks")
            assert want_counts[C:].sum() > 0 and want_out.any()


def test_colour_ring_wraps(cuda, frames):
    _, poses, depths = frames
    cfg = capi.make_config(DIMS, VS, ORIGIN)
    with capi.Volume(cfg) as ring, capi.Volume(cfg) as direct:
        ring.colour_enable()
        direct.colour_enable()
        for k, (c2w, d) in enumerate(zip(poses, depths)):
            rgb = rgb_image(k)
            ring.integrate_rgbd(d, rgb, c2w)                        # no wait between calls: a slot's refill is the ring's to order
            d_dev, c_dev = cuda.from_numpy(d).cuda(), cuda.from_numpy(rgb).cuda()
            direct.integrate_device(d_dev.data_ptr(), c2w)
            direct.integrate_colour_device(d_dev.data_ptr(), c_dev.data_ptr(), c2w)
            direct.sync()
        got, want = ring.download(), direct.download()
        assert want[1].max() >= 5
        same(got[0].view(np.uint32), want[0].view(np.uint32), "TSDF")
        same(got[1], want[1], "weights")
        c = ring.download_colour()
        assert np.count_nonzero(c) > 100
        same(c, direct.download_colour(), "packed colours")


def test_batch_parameter_ring_wraps(cuda, frames):
    """Seven undeferred frames through a two-member batch (one member masked) against per-member integration."""
    _, poses, depths = frames
    cfgs = two_members()
    mask = np.zeros((480, 640), np.uint8)
    mask[40:440, 120:520] = 255
    m_dev = cuda.from_numpy(mask).cuda()
    d_dev = [cuda.from_numpy(d).cuda() for d in depths]
    with capi.Batch(cfgs) as batch, capi.Volume(cfgs[0]) as v0, capi.Volume(cfgs[1]) as v1:
        batch.volumes[0].set_deferral(0)                            # one batched launch per frame: a slot of the ring each
        for c2w, d in zip(poses, d_dev):
            batch.integrate_device(d.data_ptr(), [m_dev.data_ptr(), None], c2w)
            v0.integrate_masked_device(d.data_ptr(), m_dev.data_ptr(), c2w)
            v1.integrate_device(d.data_ptr(), c2w)
        batch.sync()
        for i, (member, alone) in enumerate(zip(batch.volumes, (v0, v1))):
            got, want = member.download(), alone.download()
            assert want[1].sum() > 1000
            same(got[0].view(np.uint32), want[0].view(np.uint32), f"member {i} TSDF")
            same(got[1], want[1], f"member {i} weights")
