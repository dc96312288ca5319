"""Association on the device (tsdf_associate_count, tsdf_batch_associate; csrc/tsdf_associate.hip.h) against its NumPy
restatement (tests/associate_spec.py):

  * the counting kernel on crafted images, word for word: member ids -1..M-1 (and ids no render writes) with M = 1, 7 and 300
    (several member tiles), K = 1, 16 and 256 masks of bytes {0, 127, 128, 255}, live depths at every edge of the rule, odd
    and aligned image sizes, pixel-random and blocky images (the wave-uniform path), a misaligned mask pointer;
  * the product call on synth.ObjectScene: objects fused into members of different grids, associated at a pose that was not
    integrated with shuffled masks and the mask of an object the batch does not hold; the counts equal the spec applied to
    tsdf_batch_raycast_device's own render;
  * an object hidden behind another (front, not assigned), an object gone from in front of the wall (behind, not assigned),
    labels that veto a match and the score that lets it back in;
  * collected frames applied first, volumes untouched, repeatable outputs and the refusals of the C ABI."""
import ctypes as C

import numpy as np
import pytest

import associate_spec as asp
from semantic_slam_amd import capi, synth

pytestmark = pytest.mark.gpu

f32 = np.float32
_torch = None


@pytest.fixture(autouse=True)
def _bind_torch(cuda):
    global _torch
    _torch = cuda


def dev(a):
    return _torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    _torch.cuda.synchronize()
    return t.cpu().numpy()


def count_params(hw, near=0.3, far=5.0, tol=0.02):
    p = capi.associate_params_default(capi.default_config(*hw))
    p.ray.near_m, p.ray.far_m, p.depth_tol_m = near, far, tol
    return p


# ------------------------------------------------------------------------------------------------------------------------
# the counting kernel on crafted images
# ------------------------------------------------------------------------------------------------------------------------
def crafted(rng, H, W, K, M, p, blocky):
    """member, rdepth, live depth [H, W] and masks [K, H, W] that visit every branch of the rule."""
    near, far, tol = f32(p.ray.near_m), f32(p.ray.far_m), f32(p.depth_tol_m)
    if blocky:   # 16 x 16 blocks of one member / class / mask value: whole waves take the uniform path
        bh, bw = (H + 15) // 16, (W + 15) // 16

        def up(a):
            return np.kron(a, np.ones((16, 16), a.dtype))[:H, :W]
    else:
        bh, bw = H, W

        def up(a):
            return a
    member = up(rng.integers(-1, M, (bh, bw)).astype(np.int32))
    rd = up(rng.uniform(0.5, 3.0, (bh, bw)).astype(f32))
    off = np.array([0.0, tol, -tol, 0.5 * tol, -0.5 * tol, 3 * tol, -3 * tol], f32)
    d = (rd + up(rng.choice(off, (bh, bw)))).astype(f32)
    masks = np.stack([up(rng.choice(np.array([0, 127, 128, 255], np.uint8), (bh, bw))) for _ in range(K)])
    if not blocky:
        n = H * W
        edges = np.array([0.0, np.nan, np.inf, -np.inf, near, far, np.nextafter(near, f32(9)), np.nextafter(far, f32(9))], f32)
        sel = rng.random(n) < 0.08
        d.ravel()[sel] = rng.choice(edges, int(sel.sum()))
        sel = rng.random(n) < 0.03
        d.ravel()[sel] = (rd.ravel()[sel] + tol).astype(f32)
        sel = rng.random(n) < 0.03
        d.ravel()[sel] = np.nextafter((rd.ravel()[sel] - tol).astype(f32), f32(-9))
        sel = rng.random(n) < 0.02
        member.ravel()[sel] = rng.choice(np.array([-7, M, M + 3], np.int32), int(sel.sum()))   # ids no render writes
    return member, rd, d, masks


def check_counts(member, rd, d, masks, M, p, masks_dev=None):
    K = masks.shape[0]
    md = dev(masks) if masks_dev is None else masks_dev
    bufs = [dev(member), dev(rd), dev(d)]       # held for the call (a freed tensor's memory goes to the next upload)
    got, ov, mk, mb = capi.associate_count(p, bufs[0].data_ptr(), bufs[1].data_ptr(), M, bufs[2].data_ptr(),
                                           md.data_ptr(), K)
    want = asp.counts(member, rd, d, masks, M, asp.from_ctypes(p))
    if not np.array_equal(got, want):
        bad = np.nonzero(got != want)[0]
        raise AssertionError(f"{bad.size} of {got.size} words differ, first {bad[:8].tolist()}: {got[bad[:8]]} vs {want[bad[:8]]}")
    return got


@pytest.mark.parametrize("M", [1, 7, 300])
@pytest.mark.parametrize("K", [1, 16, 256])
@pytest.mark.parametrize("hw", [(37, 53), (48, 64), (61, 90)], ids=["37x53", "48x64", "61x90"])
@pytest.mark.parametrize("blocky", [False, True], ids=["pixels", "blocks"])
def test_count_parity(M, K, hw, blocky):
    rng = np.random.default_rng(M * 1000 + K * 10 + hw[0] + blocky)
    p = count_params(hw)
    member, rd, d, masks = crafted(rng, *hw, K, M, p, blocky)
    got = check_counts(member, rd, d, masks, M, p)
    ov, mk, mb = asp.split(got, K, M)
    assert mk[:, 0].sum() > 0 and mb.sum() > 0


@pytest.mark.parametrize("blocky", [False, True], ids=["pixels", "blocks"])
def test_count_parity_full_frame(blocky):
    """640 x 480: more quads than one pass of the grid, so lanes walk the grid stride."""
    rng = np.random.default_rng(11 + blocky)
    p = count_params((480, 640))
    member, rd, d, masks = crafted(rng, 480, 640, 16, 7, p, blocky)
    check_counts(member, rd, d, masks, 7, p)


def test_count_parity_misaligned_masks():
    """An aligned image size with a mask pointer one byte off: the kernel reads the masks byte by byte."""
    rng = np.random.default_rng(5)
    p = count_params((48, 64))
    member, rd, d, masks = crafted(rng, 48, 64, 5, 9, p, False)
    buf = dev(np.concatenate([np.zeros(1, np.uint8), masks.ravel()]))
    check_counts(member, rd, d, masks, 9, p, masks_dev=buf[1:])


# ------------------------------------------------------------------------------------------------------------------------
# the product call on the object scene
# ------------------------------------------------------------------------------------------------------------------------
VOXELS = (0.006, 0.008, 0.005, 0.007)
FUSED_POSES = range(0, 16, 2)
POSE = 5                                        # not integrated


def member_config(scene, i, margin=0.06):
    lo, hi = scene.bounds(i)
    vs = VOXELS[i % len(VOXELS)]
    lo = lo - margin
    dims = np.ceil((hi + margin - lo) / vs).astype(int) + 1
    dims[0] = (dims[0] + 3) // 4 * 4            # batch members: dim_x % 4 == 0
    return capi.make_config(tuple(int(x) for x in dims), vs, lo.astype(f32), vol_id=i)


def fuse(batch, scene, objects, poses=FUSED_POSES):
    """Frames of `scene` at `poses`, each member fed depth x its object's mask."""
    for k in poses:
        c = scene.pose(k)
        ids = scene.ids(c)
        d = dev(scene.depth(c))
        ms = [dev(np.where(ids == o, 255, 0).astype(np.uint8)) for o in objects]
        batch.integrate_device(d.data_ptr(), [m.data_ptr() for m in ms], c)
        _torch.cuda.synchronize()


def render(batch, pose, p):
    d = _torch.empty(480 * 640, dtype=_torch.float32, device="cuda")      # written on the batch's stream
    m = _torch.empty(480 * 640, dtype=_torch.int32, device="cuda")
    batch.raycast_device(pose, d.data_ptr(), None, m.data_ptr(), params=p.ray)
    return host(m).reshape(480, 640), host(d).reshape(480, 640)


@pytest.fixture(scope="module")
def scene_batch(cuda):
    scene = synth.ObjectScene()
    objects = [0, 1, 2]                          # object 3 is not in the batch
    cfgs = [member_config(scene, o) for o in objects]
    batch = capi.Batch(cfgs)
    fuse(batch, scene, objects)
    batch.sync()
    yield scene, objects, cfgs, batch
    batch.close()


def masks_of(ids, objs):
    return np.stack([np.where(ids == o, 255, 0).astype(np.uint8) for o in objs])


def test_end_to_end_permutation_and_spec(scene_batch):
    scene, objects, cfgs, batch = scene_batch
    pose = scene.pose(POSE)
    ids = scene.ids(pose)
    live = scene.depth(pose)
    order = [2, 3, 0, 1]                         # shuffled, and object 3 is no member
    masks = masks_of(ids, order)
    p = capi.associate_params_default(cfgs[0])
    d_live, d_masks = dev(live), dev(masks)
    out = batch.associate(pose, d_live.data_ptr(), d_masks.data_ptr(), len(order), params=p)
    want_assign = [objects.index(o) if o in objects else -1 for o in order]
    assert out["assign"].tolist() == want_assign, (out["assign"], out["iou"])
    assert (out["iou"][np.array(want_assign) >= 0] > 0.5).all(), out["iou"]
    member, rdepth = render(batch, pose, p)
    want = asp.counts(member, rdepth, live, masks, len(objects), asp.from_ctypes(p))
    assert np.array_equal(out["counts"], want)
    a, iou = asp.assign(want, len(order), len(objects), asp.from_ctypes(p))
    assert a.tolist() == out["assign"].tolist() and iou.tobytes() == out["iou"].tobytes()
    # the mask of the object no member holds is the part of the frame no object explains
    assert out["mask"][1, 2] > 0.9 * out["mask"][1, 1] and out["overlap"][1, :, 0].sum() < p.min_pixels


def test_labels_veto_and_score(scene_batch):
    scene, objects, cfgs, batch = scene_batch
    pose = scene.pose(POSE)
    order = [2, 3, 0, 1]
    masks = dev(masks_of(scene.ids(pose), order))
    d_live = dev(scene.depth(pose))
    member_label, member_score = np.array([11, 12, 13], np.uint16), np.array([0.9, 0.9, 0.9], f32)
    mask_label, mask_score = np.array([13, 14, 11, 12], np.uint16), np.array([0.9, 0.9, 0.9, 0.9], f32)

    def run(ml, bs):
        return batch.associate(pose, d_live.data_ptr(), masks.data_ptr(), 4,
                               labels=(ml, mask_score, member_label, bs))["assign"].tolist()

    assert run(mask_label, member_score) == [2, -1, 0, 1]
    vetoed = mask_label.copy()
    vetoed[2] = 99                               # the mask of object 0 now says another class, with the same score
    assert run(vetoed, member_score) == [2, -1, -1, 1]
    back = member_score.copy()
    back[0] = 1.0                                # 1.0 > 1.1f * 0.9f: the member's confidence lets it back in
    assert run(vetoed, back) == [2, -1, 0, 1]


def test_hidden_object_is_in_front_and_not_assigned(cuda):
    scene = synth.ObjectScene()
    cfgs = [member_config(scene, 0)]
    with capi.Batch(cfgs) as batch:
        fuse(batch, scene, [0])
        pose = scene.pose(POSE)
        T = pose.reshape(4, 4).astype(np.float64)
        cam, c0 = T[:3, 3], np.asarray(synth.OBJECTS[0][1])
        occluder = ("sphere", tuple(cam + 0.6 * (c0 - cam)), 0.1)
        live_scene = synth.ObjectScene(synth.OBJECTS + (occluder,))
        ids = live_scene.ids(pose)
        assert (ids == 0).sum() == 0                                  # object 0 is hidden
        masks = dev(masks_of(ids, [4]))
        live = dev(live_scene.depth(pose))
        out = batch.associate(pose, live.data_ptr(), masks.data_ptr(), 1)
        agree, front, behind = out["overlap"][0, 0].tolist()
        assert agree == 0 and front > 1000, out["overlap"]
        assert out["assign"].tolist() == [-1] and out["iou"][0] == 0.0


def test_object_gone_from_the_wall_is_behind_and_not_assigned(cuda):
    scene = synth.ObjectScene()
    cfgs = [member_config(scene, 0)]
    with capi.Batch(cfgs) as batch:
        fuse(batch, scene, [0])
        pose = scene.pose(POSE)
        p = capi.associate_params_default(cfgs[0])
        member, _ = render(batch, pose, p)
        assert (member == 0).sum() > 1000
        gone = synth.ObjectScene(synth.OBJECTS[1:])                  # the camera now sees the wall where object 0 was
        masks = dev(np.where(member == 0, 255, 0).astype(np.uint8)[None])
        live = dev(gone.depth(pose))
        out = batch.associate(pose, live.data_ptr(), masks.data_ptr(), 1, params=p)
        agree, front, behind = out["overlap"][0, 0].tolist()
        assert agree == 0 and front == 0 and behind == (member == 0).sum(), out["overlap"]
        assert out["member"][0, 2] == behind
        assert out["assign"].tolist() == [-1]


# ------------------------------------------------------------------------------------------------------------------------
# call semantics
# ------------------------------------------------------------------------------------------------------------------------
def test_collected_frames_read_only_and_repeatable(cuda):
    scene = synth.ObjectScene()
    objects = [0, 2]
    cfgs = [member_config(scene, o) for o in objects]
    pose = scene.pose(POSE)
    ids = scene.ids(pose)
    masks = dev(masks_of(ids, [0, 2, 1]))
    live = dev(scene.depth(pose))
    with capi.Batch(cfgs) as ref:
        ref.volumes[0].set_deferral(0)
        fuse(ref, scene, objects)
        ref.sync()
        want = ref.associate(pose, live.data_ptr(), masks.data_ptr(), 3)
    assert want["assign"].tolist() == [0, 1, -1]
    with capi.Batch(cfgs) as b:
        b.volumes[0].set_deferral(32)            # frames are collected, and the call applies them first
        keep = []                                # the frames stay allocated until the batch's stream has copied them
        for k in FUSED_POSES:
            c = scene.pose(k)
            i = scene.ids(c)
            d = dev(scene.depth(c))
            ms = [dev(np.where(i == o, 255, 0).astype(np.uint8)) for o in objects]
            b.integrate_device(d.data_ptr(), [m.data_ptr() for m in ms], c)
            keep.append((d, ms))
        got = b.associate(pose, live.data_ptr(), masks.data_ptr(), 3)
        assert got["counts"].tobytes() == want["counts"].tobytes()
        assert got["assign"].tobytes() == want["assign"].tobytes() and got["iou"].tobytes() == want["iou"].tobytes()
        before = [v.download() for v in b.volumes]
        again = b.associate(pose, live.data_ptr(), masks.data_ptr(), 3)
        after = [v.download() for v in b.volumes]
        for (t0, w0), (t1, w1) in zip(before, after):
            assert t0.tobytes() == t1.tobytes() and w0.tobytes() == w1.tobytes()
        for key in ("counts", "assign", "iou"):
            assert again[key].tobytes() == got[key].tobytes(), key


def test_refusals(cuda):
    lib = capi.load()
    cfg = capi.make_config((32, 32, 32), 0.01, [-0.16, -0.16, 1.0])
    depth = _torch.zeros(480 * 640, dtype=_torch.float32, device="cuda")
    masks = _torch.zeros(2 * 480 * 640, dtype=_torch.uint8, device="cuda")
    _torch.cuda.synchronize()                    # the fills ran before the batch's stream reads them
    eye = np.eye(4, dtype=f32).ravel()
    a, i = np.zeros(257, np.int32), np.zeros(257, f32)
    with capi.Batch([cfg, cfg]) as batch:
        good = capi.associate_params_default(cfg)

        def refused(p, what, b=batch._h, pose=eye, d=depth.data_ptr(), m=masks.data_ptr(), k=2, labels=None, ao=a, io=i):
            rc = lib.tsdf_batch_associate(b, C.byref(p) if p is not None else None,
                                          pose.ctypes.data if pose is not None else None, d, m, k, labels, None,
                                          ao.ctypes.data if ao is not None else None, io.ctypes.data if io is not None else None)
            msg = lib.tsdf_last_error().decode()
            assert rc == -1 and what in msg, (rc, msg)

        refused(good, "NULL", b=None)
        refused(None, "NULL parameters")
        refused(good, "NULL", pose=None)
        refused(good, "NULL", d=None)
        refused(good, "NULL", m=None)
        refused(good, "NULL", ao=None)
        refused(good, "NULL", io=None)
        refused(good, "k = 0", k=0)
        refused(good, "k = 257", k=257)
        for field, value, what in (("depth_tol_m", 0.0, "depth_tol_m"), ("depth_tol_m", float("nan"), "depth_tol_m"),
                                   ("min_pixels", 0, "min_pixels"), ("min_iou", 1.01, "min_iou"),
                                   ("min_iou", float("nan"), "min_iou"), ("one_to_one", -1, "one_to_one")):
            p = capi.associate_params_default(cfg)
            setattr(p, field, value)
            refused(p, what)
        for field, value, what in (("near_m", -1.0, "near"), ("far_m", 0.0, "near"), ("im_height", 240, "render is"),
                                   ("im_width", 320, "render is"), ("im_height", 0, "image size")):
            p = capi.associate_params_default(cfg)
            setattr(p.ray, field, value)
            refused(p, what)
        lab = capi.AssociateLabels(None, None, None, None)
        refused(good, "label block", labels=C.byref(lab))
        out = batch.associate(eye, depth.data_ptr(), masks.data_ptr(), 2)     # and a good call still works
        assert out["assign"].tolist() == [-1, -1] and out["member"].sum() == 0
    p = count_params((48, 64))
    buf = _torch.zeros(48 * 64, dtype=_torch.float32, device="cuda")
    counts = np.zeros(asp.n_words(2, 3), np.uint32)
    for args, what in (((None, buf, 3, buf, masks, 2), "NULL"), ((buf, buf, 0, buf, masks, 2), "n_members = 0"),
                       ((buf, buf, 65537, buf, masks, 2), "n_members = 65537"), ((buf, buf, 3, buf, masks, 0), "k = 0")):
        ptrs = [x.data_ptr() if hasattr(x, "data_ptr") else x for x in args]
        rc = lib.tsdf_associate_count(0, C.byref(p), ptrs[0], ptrs[1], ptrs[2], ptrs[3], ptrs[4], ptrs[5], counts.ctypes.data)
        msg = lib.tsdf_last_error().decode()
        assert rc == -1 and what in msg, (rc, msg)
