"""Geometric segmentation and mask refinement on the device (tsdf_segment_depth_device, tsdf_segment_refine_masks_device,
tsdf_segment_frame; csrc/tsdf_segment.hip.h) against the NumPy restatement (tests/segment_spec.py).  Every comparison is for
equality of all bits: the DoN image (float32 words), the cluster image, n_clusters, the count block and the refined masks.

  * image sizes 640 x 480, 320 x 240 (K halved), 161 x 97 and 1 x 1;
  * frames: synth.ObjectScene poses; the same scene standing on a floor box (objects touch their support: at threshold 0.25
    every object is a cluster of its own, at 0.1 two merge with the floor); sensor noise and holes; NaN, inf and negative depth;
  * sweeps over both radii, the DoN and overlap thresholds, seg_radius, the size filter, inset 0..3 and K in {1, 4, 64};
  * the refinement alone on random caller-made cluster images (labels outside 1..C included);
  * a caller's stream, inputs unchanged, repeatable outputs, the refusals;
  * tsdf_batch_associate fed the refined masks of bled instance masks gives the assignment the ground-truth masks give."""
import ctypes as C

import numpy as np
import pytest

import segment_spec as ss
from semantic_slam_amd import capi, synth

pytestmark = pytest.mark.gpu

f32 = np.float32
_torch = None
FLOOR = ("box", (-2, .32, .3), (2, .40, 3))


@pytest.fixture(autouse=True)
def _bind_torch(cuda):
    global _torch
    _torch = cuda


def dev(a):
    return _torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    _torch.cuda.synchronize()
    return t.cpu().numpy()


def camera(scale):
    K = np.array(synth.TUM_K, np.float64)
    K[[0, 2, 4, 5]] /= scale
    return K


def scene_at(scale, hw, objects=synth.OBJECTS):
    return synth.ObjectScene(objects=objects, K=camera(scale), h=hw[0], w=hw[1])


def lib_params(hw, K, **kw):
    cfg = capi.default_config(*hw)
    cfg.cam_K[:] = [float(x) for x in np.asarray(K, f32)]
    p = capi.segment_params_default(cfg)
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def dilate(m, r):
    h, w = m.shape
    pad = np.zeros((h + 2 * r, w + 2 * r), bool)
    pad[r:r + h, r:r + w] = m
    out = np.zeros((h, w), bool)
    for dy in range(2 * r + 1):
        for dx in range(2 * r + 1):
            out |= pad[dy:dy + h, dx:dx + w]
    return out


def bled_masks(ids, n, r):
    return np.stack([np.where(dilate(ids == i, r), 255, 0).astype(np.uint8) for i in range(n)])


def random_masks(rng, K, hw):
    """K masks of random rectangles with bytes around 128."""
    H, W = hw
    m = np.zeros((K, H, W), np.uint8)
    for k in range(K):
        for _ in range(int(rng.integers(1, 4))):
            y0, x0 = int(rng.integers(0, H)), int(rng.integers(0, W))
            y1, x1 = y0 + int(rng.integers(1, H // 2 + 2)), x0 + int(rng.integers(1, W // 2 + 2))
            m[k, y0:y1, x0:x1] = rng.choice(np.array([128, 200, 255], np.uint8))
        holes = rng.random((H, W)) < 0.002
        m[k][holes] = rng.choice(np.array([0, 127], np.uint8), int(holes.sum()))
    return m


_values = {}


def spec_values(key, depth, sp):
    """The threshold-independent part of the spec's DoN, kept per (frame, camera, range, radii): sweeps share it."""
    k = (key, sp.H, sp.W, float(sp.near_m), float(sp.far_m), float(sp.small_radius_m), float(sp.large_radius_m))
    if k not in _values:
        _values[k] = ss.don_values(depth, sp)
    return _values[k]


def differ(name, got, want):
    if got.tobytes() != want.tobytes():
        bad = np.nonzero(got.ravel().view(np.uint8 if got.dtype == np.uint8 else np.uint32) !=
                         want.ravel().view(np.uint8 if want.dtype == np.uint8 else np.uint32))[0]
        raise AssertionError(f"{name}: {bad.size} of {got.size} words differ, first {bad[:6].tolist()}: "
                             f"{got.ravel()[bad[:6]]} vs {want.ravel()[bad[:6]]}")


def check_depth(seg, p, depth, key):
    """Runs tsdf_segment_depth_device and holds DoN, clusters and their number to the spec; returns (cluster, C)."""
    H, W = p.im_height, p.im_width
    sp = ss.from_ctypes(p)
    d_depth = dev(depth)
    d_don = _torch.full((H, W), -7.0, dtype=_torch.float32, device="cuda")
    d_cl = _torch.full((H, W), -7, dtype=_torch.int32, device="cuda")
    n = seg.segment_depth(p, d_depth.data_ptr(), d_cl.data_ptr(), d_don.data_ptr())
    want_don, want_cl, want_n = ss.segment_depth(depth, sp, spec_values(key, depth, sp))
    differ("DoN", host(d_don), want_don)
    differ("clusters", host(d_cl), want_cl)
    assert n == want_n
    assert host(d_depth).tobytes() == np.ascontiguousarray(depth, f32).tobytes()      # the input is only read
    return want_cl, want_n


def check_refine(seg, p, cluster, n, masks):
    K = masks.shape[0]
    d_cl, d_m = dev(np.ascontiguousarray(cluster, np.int32)), dev(masks)
    d_out = _torch.full(masks.shape, 77, dtype=_torch.uint8, device="cuda")
    size, inside = seg.refine_masks(p, d_cl.data_ptr(), n, d_m.data_ptr(), K, d_out.data_ptr())
    want_out, want_counts = ss.refine(cluster, n, masks, ss.from_ctypes(p))
    differ("counts", np.concatenate([size, inside.ravel()]), want_counts)
    differ("refined masks", host(d_out), want_out)
    assert host(d_m).tobytes() == masks.tobytes() and host(d_cl).tobytes() == np.ascontiguousarray(cluster, np.int32).tobytes()
    return want_out


def check_frame(seg, p, depth, masks, key):
    K = masks.shape[0]
    sp = ss.from_ctypes(p)
    d_depth, d_m = dev(depth), dev(masks)
    d_out = _torch.full(masks.shape, 77, dtype=_torch.uint8, device="cuda")
    d_cl = _torch.full((p.im_height, p.im_width), -7, dtype=_torch.int32, device="cuda")
    n = seg.segment_frame(p, d_depth.data_ptr(), d_m.data_ptr(), K, d_out.data_ptr(), d_cl.data_ptr())
    _, want_cl, want_n = ss.segment_depth(depth, sp, spec_values(key, depth, sp))
    want_out, _ = ss.refine(want_cl, want_n, masks, sp)
    assert n == want_n
    differ("clusters", host(d_cl), want_cl)
    differ("refined masks", host(d_out), want_out)
    d_out2 = _torch.full(masks.shape, 77, dtype=_torch.uint8, device="cuda")
    assert seg.segment_frame(p, d_depth.data_ptr(), d_m.data_ptr(), K, d_out2.data_ptr()) == n      # no cluster image asked
    differ("refined masks without a cluster image", host(d_out2), want_out)
    return want_out, want_cl, n


# ------------------------------------------------------------------------------------------------------------------------
# frames and image sizes
# ------------------------------------------------------------------------------------------------------------------------
HALF = (240, 320)


@pytest.fixture(scope="module")
def seg_half(cuda):
    with capi.Segmenter(*HALF) as s:
        yield s


@pytest.mark.parametrize("pose", [0, 3, 5])
def test_object_scene_half_size(seg_half, pose):
    scene = scene_at(2, HALF)
    c = scene.pose(pose)
    depth, ids = scene.depth(c), scene.ids(c)
    p = lib_params(HALF, camera(2))
    masks = bled_masks(ids, 4, 3)
    out, cl, n = check_frame(seg_half, p, depth, masks, ("obj", pose))
    assert n >= 4
    check_depth(seg_half, p, depth, ("obj", pose))
    check_refine(seg_half, p, cl, n, masks)
    for i in range(4):
        assert ((out[i] == 255) & (ids != i)).sum() == 0 and (out[i] == 255).sum() > 0.8 * (ids == i).sum()


def test_full_size_frame(cuda):
    scene = synth.ObjectScene()
    c = scene.pose(3)
    depth, ids = scene.depth(c), scene.ids(c)
    p = lib_params((480, 640), synth.TUM_K)
    masks = bled_masks(ids, 4, 6)
    with capi.Segmenter(480, 640) as seg:
        cl, n = check_depth(seg, p, depth, ("full", 3))
        out = check_refine(seg, p, cl, n, masks)
    for i in range(4):
        o, true = out[i] == 255, ids == i
        assert (o & ~true).sum() == 0 and (o & true).sum() >= 0.9 * true.sum()


@pytest.mark.parametrize("thresh,separate", [(0.25, True), (0.1, False)])
def test_objects_on_a_floor(seg_half, thresh, separate):
    scene = scene_at(2, HALF, synth.OBJECTS + (FLOOR,))
    c = scene.pose(3)
    depth, ids = scene.depth(c), scene.ids(c)
    p = lib_params(HALF, camera(2), don_thresh=thresh)
    cl, n = check_depth(seg_half, p, depth, ("floor", 3))
    check_refine(seg_half, p, cl, n, bled_masks(ids, 5, 3))
    main = []
    for i in range(4):                                          # the cluster most of object i lies in
        labels = cl[(ids == i) & (cl > 0)]
        main.append(int(np.bincount(labels).argmax()))
    print("threshold", thresh, "clusters", n, "main cluster per object", main)
    if separate:
        assert len(set(main)) == 4


def test_noise_and_holes(seg_half):
    scene = scene_at(2, HALF)
    c = scene.pose(1)
    depth = synth.sensor_imperfections([scene.depth(c)], noise_mm=2.0, holes=0.05, seed=7)[0]
    p = lib_params(HALF, camera(2))
    cl, n = check_depth(seg_half, p, depth, ("noise", 1))
    check_refine(seg_half, p, cl, n, bled_masks(scene.ids(c), 4, 3))
    p2 = lib_params(HALF, camera(2), min_cluster=1, seg_radius_m=0.004)     # below the pixel spacing: a cluster per kept pixel
    cl2, n2 = check_depth(seg_half, p2, depth, ("noise", 1))
    assert n2 > 100 * n
    check_refine(seg_half, p2, cl2, n2, random_masks(np.random.default_rng(2), 4, HALF))


def test_invalid_depth_values(seg_half):
    scene = scene_at(2, HALF)
    rng = np.random.default_rng(5)
    depth = scene.depth(scene.pose(2)).copy()
    sel = rng.random(depth.shape) < 0.03
    depth[sel] = rng.choice(np.array([np.nan, np.inf, -np.inf, -1.0, 0.0, 0.3, 5.5, 40.0], f32), int(sel.sum()))
    depth[100:110, 50:200] = np.nan
    p = lib_params(HALF, camera(2), near_m=0.3, far_m=5.0)
    cl, n = check_depth(seg_half, p, depth, ("invalid", 2))
    assert n >= 1


@pytest.mark.parametrize("hw,scale", [((97, 161), 4), ((1, 1), 4), ((1, 40), 4), ((33, 2), 4)],
                         ids=["161x97", "1x1", "40x1", "2x33"])
def test_odd_sizes(cuda, hw, scale):
    K = camera(scale)
    p = lib_params(hw, K, min_cluster=3)
    if hw == (97, 161):
        scene = scene_at(scale, hw)
        depth = scene.depth(scene.pose(4))
        masks = bled_masks(scene.ids(scene.pose(4)), 4, 2)
    else:
        rng = np.random.default_rng(hw[0] + hw[1])
        depth = rng.uniform(0.9, 1.1, hw).astype(f32)
        masks = random_masks(rng, 3, hw)
    with capi.Segmenter(*hw) as seg:
        cl, n = check_depth(seg, p, depth, ("odd", hw))
        check_refine(seg, p, cl, n, masks)
        check_frame(seg, p, depth, masks, ("odd", hw))


# ------------------------------------------------------------------------------------------------------------------------
# parameter sweeps
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("small,large", [(0.03, 0.5), (0.08, 0.5), (0.05, 0.3), (0.05, 0.9), (0.02, 0.1)])
def test_radius_sweep(seg_half, small, large):
    scene = scene_at(2, HALF)
    depth = scene.depth(scene.pose(6))
    p = lib_params(HALF, camera(2), small_radius_m=small, large_radius_m=large)
    check_depth(seg_half, p, depth, ("obj", 6))


@pytest.mark.parametrize("don_thresh", [0.02, 0.25, 0.6])
@pytest.mark.parametrize("seg_radius", [0.004, 0.02, 0.2])
def test_threshold_and_seg_radius_sweep(seg_half, don_thresh, seg_radius):
    scene = scene_at(2, HALF)
    depth = scene.depth(scene.pose(0))
    for lo, hi in ((15, 1000000), (1, 400), (300, 2000)):
        p = lib_params(HALF, camera(2), don_thresh=don_thresh, seg_radius_m=seg_radius, min_cluster=lo, max_cluster=hi)
        check_depth(seg_half, p, depth, ("obj", 0))


@pytest.mark.parametrize("K", [1, 4, 64])
@pytest.mark.parametrize("inset", [0, 1, 2, 3])
def test_inset_overlap_and_mask_count_sweep(seg_half, K, inset):
    scene = scene_at(2, HALF)
    c = scene.pose(0)
    depth, ids = scene.depth(c), scene.ids(c)
    sp = ss.from_ctypes(lib_params(HALF, camera(2)))
    _, cl, n = ss.segment_depth(depth, sp, spec_values(("obj", 0), depth, sp))
    rng = np.random.default_rng(K * 10 + inset)
    masks = np.concatenate([bled_masks(ids, 4, 3), random_masks(rng, 60, HALF)])[:K]
    if K == 1:
        masks = bled_masks(ids, 4, 3)[2:3]
    for overlap in (0.05, 0.5, 0.95, 1.0):
        p = lib_params(HALF, camera(2), inset=inset, overlap=overlap)
        check_refine(seg_half, p, cl, n, masks)


@pytest.mark.parametrize("hw", [(48, 64), (61, 90)], ids=["64x48", "90x61"])
@pytest.mark.parametrize("blocky", [False, True], ids=["pixels", "blocks"])
def test_refine_on_caller_made_cluster_images(cuda, hw, blocky):
    rng = np.random.default_rng(hw[0] + blocky)
    H, W = hw
    with capi.Segmenter(H, W) as seg:
        for n, K in ((1, 1), (5, 3), (40, 16), (300, 7), (3, 256)):
            if blocky:
                cl = np.kron(rng.integers(0, n + 1, ((H + 7) // 8, (W + 7) // 8)), np.ones((8, 8), np.int64))[:H, :W]
            else:
                cl = rng.integers(0, n + 1, (H, W))
            cl = cl.astype(np.int32)
            sel = rng.random((H, W)) < 0.02
            cl[sel] = rng.choice(np.array([-1, -5, n + 1, n + 9, 2 ** 30], np.int32), int(sel.sum()))   # none of these is a label
            masks = random_masks(rng, K, hw)
            for inset in (0, 1, 2):
                check_refine(seg, lib_params(hw, camera(8), inset=inset, overlap=0.3), cl, n, masks)
        check_refine(seg, lib_params(hw, camera(8)), np.zeros(hw, np.int32), 0, random_masks(rng, 2, hw))   # no cluster at all


# ------------------------------------------------------------------------------------------------------------------------
# streams, repeatability, refusals
# ------------------------------------------------------------------------------------------------------------------------
def test_caller_stream_and_repeatability(cuda):
    scene = scene_at(2, HALF)
    c = scene.pose(7)
    depth, ids = scene.depth(c), scene.ids(c)
    masks = bled_masks(ids, 4, 3)
    p = lib_params(HALF, camera(2))
    stream = cuda.cuda.Stream()
    with capi.Segmenter(*HALF) as seg:
        first = check_frame(seg, p, depth, masks, ("obj", 7))
        seg.set_stream(stream.cuda_stream)
        second = check_frame(seg, p, depth, masks, ("obj", 7))
        check_depth(seg, p, depth, ("obj", 7))
        seg.set_stream(None)
        third = check_frame(seg, p, depth, masks, ("obj", 7))
    assert first[2] == second[2] == third[2]


def test_refusals_with_a_segmenter(cuda):
    lib = capi.load()
    p = lib_params(HALF, camera(2))
    d_depth = dev(np.ones(HALF, f32))
    d_cl = _torch.zeros(HALF, dtype=_torch.int32, device="cuda")
    d_m = _torch.zeros((2,) + HALF, dtype=_torch.uint8, device="cuda")
    d_o = _torch.zeros((2,) + HALF, dtype=_torch.uint8, device="cuda")
    n = C.c_int32()
    with capi.Segmenter(*HALF) as seg:
        h = seg._h

        def refused(rc, what):
            msg = lib.tsdf_last_error().decode()
            assert rc == -1 and what in msg, (rc, msg)

        pp = C.byref(p)
        refused(lib.tsdf_segment_depth_device(h, pp, None, None, d_cl.data_ptr(), C.byref(n)), "NULL")
        refused(lib.tsdf_segment_depth_device(h, pp, d_depth.data_ptr(), None, None, C.byref(n)), "NULL")
        refused(lib.tsdf_segment_depth_device(h, pp, d_depth.data_ptr(), None, d_cl.data_ptr(), None), "NULL")
        refused(lib.tsdf_segment_refine_masks_device(h, pp, None, 1, d_m.data_ptr(), 2, d_o.data_ptr(), None), "NULL")
        refused(lib.tsdf_segment_refine_masks_device(h, pp, d_cl.data_ptr(), 1, None, 2, d_o.data_ptr(), None), "NULL")
        refused(lib.tsdf_segment_refine_masks_device(h, pp, d_cl.data_ptr(), 1, d_m.data_ptr(), 2, None, None), "NULL")
        refused(lib.tsdf_segment_refine_masks_device(h, pp, d_cl.data_ptr(), 1, d_m.data_ptr(), 2, d_m.data_ptr(), None), "in place")
        refused(lib.tsdf_segment_refine_masks_device(h, pp, d_cl.data_ptr(), 1 << 23, d_m.data_ptr(), 2, d_o.data_ptr(), None),
                "count block")                                  # 2^23 + 2^23 * 2 words are above 2^24
        refused(lib.tsdf_segment_frame(h, pp, None, d_m.data_ptr(), 2, d_o.data_ptr(), None, C.byref(n)), "NULL")
        refused(lib.tsdf_segment_frame(h, pp, d_depth.data_ptr(), d_m.data_ptr(), 2, d_o.data_ptr(), None, None), "NULL")
        refused(lib.tsdf_segment_frame(h, pp, d_depth.data_ptr(), d_m.data_ptr(), 2, d_m.data_ptr(), None, C.byref(n)), "in place")
        refused(lib.tsdf_segment_frame(h, pp, d_depth.data_ptr(), d_m.data_ptr(), 0, d_o.data_ptr(), None, C.byref(n)), "k = 0")
        other = lib_params((480, 640), synth.TUM_K)
        refused(lib.tsdf_segment_depth_device(h, C.byref(other), d_depth.data_ptr(), None, d_cl.data_ptr(), C.byref(n)),
                "the segmenter's")
        refused(lib.tsdf_segment_frame(h, C.byref(other), d_depth.data_ptr(), d_m.data_ptr(), 2, d_o.data_ptr(), None, C.byref(n)),
                "the segmenter's")
        bad = lib_params(HALF, camera(2), small_radius_m=0.5)
        refused(lib.tsdf_segment_depth_device(h, C.byref(bad), d_depth.data_ptr(), None, d_cl.data_ptr(), C.byref(n)),
                "below large_radius_m")
        assert seg.segment_depth(p, d_depth.data_ptr(), d_cl.data_ptr()) == 0        # and a good call still works: a plane
        assert not host(d_cl).any()


# ------------------------------------------------------------------------------------------------------------------------
# association fed refined masks
# ------------------------------------------------------------------------------------------------------------------------
VOXELS = (0.006, 0.008, 0.005, 0.007)


def member_config(scene, i, margin=0.06):
    lo, hi = scene.bounds(i)
    vs = VOXELS[i % len(VOXELS)]
    lo = lo - margin
    dims = np.ceil((hi + margin - lo) / vs).astype(int) + 1
    dims[0] = (dims[0] + 3) // 4 * 4
    return capi.make_config(tuple(int(x) for x in dims), vs, lo.astype(f32), vol_id=i)


def test_association_with_refined_masks(cuda):
    scene = synth.ObjectScene()
    objects = [0, 1, 2]                                         # object 3 is not in the batch
    cfgs = [member_config(scene, o) for o in objects]
    order = [2, 3, 0, 1]
    pose = scene.pose(5)
    ids, live = scene.ids(pose), scene.depth(pose)
    truth = np.stack([np.where(ids == o, 255, 0).astype(np.uint8) for o in order])
    bled = np.stack([np.where(dilate(ids == o, 6), 255, 0).astype(np.uint8) for o in order])
    with capi.Batch(cfgs) as batch, capi.Segmenter(480, 640) as seg:
        for k in range(0, 16, 2):
            c = scene.pose(k)
            kid = scene.ids(c)
            d = dev(scene.depth(c))
            ms = [dev(np.where(kid == o, 255, 0).astype(np.uint8)) for o in objects]
            batch.integrate_device(d.data_ptr(), [m.data_ptr() for m in ms], c)
            _torch.cuda.synchronize()
        batch.sync()
        d_live, d_truth, d_bled = dev(live), dev(truth), dev(bled)
        d_ref = _torch.zeros(bled.shape, dtype=_torch.uint8, device="cuda")
        n = seg.segment_frame(capi.segment_params_default(cfgs[0]), d_live.data_ptr(), d_bled.data_ptr(), 4, d_ref.data_ptr())
        assert n >= 4
        refined = host(d_ref)
        for j, o in enumerate(order):
            assert ((refined[j] == 255) & (ids != o)).sum() == 0
        want = batch.associate(pose, d_live.data_ptr(), d_truth.data_ptr(), 4)
        got = batch.associate(pose, d_live.data_ptr(), d_ref.data_ptr(), 4)
        assert want["assign"].tolist() == [2, -1, 0, 1]
        assert got["assign"].tolist() == want["assign"].tolist(), (got["assign"], got["iou"])
