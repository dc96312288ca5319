"""Raycasting on the device (csrc/tsdf_raycast.hip.h) against its float32 restatement (tests/raycast_spec.py), bit for bit:
depth, normal, label, colour and batch member, over grid shapes, render sizes, intrinsics, the default / fused-sequence /
masked Integrate paths and uploaded states with NaN, +-inf, +-0 and weights at the threshold; plus ordering (deferred frames,
caller streams), read-only-ness, the batch's nearest-member rule and the refusals of the C ABI.  (No output is ever NaN under
the rule, so every comparison is of all 32 bits.)"""
import ctypes as C

import numpy as np
import pytest

import raycast_spec as rs
from fuzz_cases import NAN_PAYLOAD
from semantic_slam_amd import capi, synth

pytestmark = pytest.mark.gpu

f32 = np.float32


def same_bits(got, want, what):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape, f"{what}: shape {got.shape} vs {want.shape}"
    g = got.view(np.uint8).reshape(got.shape + (-1,))
    w = want.view(np.uint8).reshape(want.shape + (-1,))
    bad = np.any(g != w, axis=-1)
    assert not bad.any(), f"{what}: {bad.sum()} of {bad.size} differ, first at {np.argwhere(bad)[:3].tolist()}"


def params(K, hw, near=0.0, far=6.0, thr=0.9):
    p = capi.RaycastParams()
    p.cam_K[:] = [float(x) for x in np.asarray(K, f32).ravel()]
    p.im_height, p.im_width = hw
    p.near_m, p.far_m, p.weight_thresh = near, far, thr
    return p


def spec(vol, t, w, p, cam2world, pixels=None, label=None, colour=None):
    c = vol.cfg
    c2b = capi.multiply_matrix(capi.invert_matrix(np.asarray(c.base2world, f32))[1], cam2world)
    return rs.render(t, w, (c.dim_x, c.dim_y, c.dim_z), np.asarray(c.origin, f32), c.voxel_size, c.trunc_margin,
                     np.asarray(p.cam_K, f32), (p.im_height, p.im_width), p.near_m, p.far_m, p.weight_thresh, c2b,
                     pixels=pixels, label=label, colour=colour)


def check_render(vol, p, cam2world, what, pixels=None, label=None, colour=None):
    t, w = vol.download()
    got = vol.raycast(cam2world, params=p, normals=True, labels=label is not None, colour=colour is not None)
    want = spec(vol, t, w, p, cam2world, pixels=pixels, label=label, colour=colour)
    sel = (slice(None),) if pixels is None else (np.asarray(pixels)[:, 1], np.asarray(pixels)[:, 0])
    pick = (lambda a: a.reshape(-1, *a.shape[2:])) if pixels is None else (lambda a: a[sel])
    same_bits(pick(got["depth"]), want["depth"], f"{what} depth")
    same_bits(pick(got["normal"]), want["normal"], f"{what} normal")
    if label is not None:
        same_bits(pick(got["label"]), want["label"], f"{what} label")
    if colour is not None:
        same_bits(pick(got["colour"]), want["colour"], f"{what} colour")
    return got, want


def surf_frames(dims, vs, origin, poses_k, n=64, K=synth.TUM_K, hw=(480, 640)):
    scene = synth.SurfScene(dims, vs, origin, K=K, h=hw[0], w=hw[1])
    poses = [scene.pose(k, n=n) for k in poses_k]
    return scene, poses, [scene.depth(c, quantize=True) for c in poses]


def volume_for(dims, edge_vs=None):
    vs = edge_vs or 0.8 / max(dims)
    origin = synth.surf_volume(max(dims), vs, 0.8)
    return capi.make_config(dims, vs, origin), vs, origin


# ------------------------------------------------------------------------------------------------------------------------
# parity over shapes, paths, render sizes and intrinsics
# ------------------------------------------------------------------------------------------------------------------------
K_OTHER = np.array([300.0, 0, 75.3, 0, 310.0, 52.1, 0, 0, 1], f32)
RENDERS = [(synth.TUM_K, (480, 640)), (K_OTHER, (97, 161)), (np.array([500.0, 0, 0.0, 0, 500.0, 0.0, 0, 0, 1], f32), (1, 1))]


@pytest.mark.parametrize("dims", [(128, 96, 64), (160, 120, 132), (256, 160, 132)])
@pytest.mark.parametrize("path", ["default", "sequence", "masked"])
def test_parity_with_the_restatement(cuda, dims, path):
    cfg, vs, origin = volume_for(dims)
    scene, poses, depths = surf_frames(dims, vs, origin, range(0, 64, 8))
    d_dev = [cuda.from_numpy(d).cuda() for d in depths]
    mask = np.zeros((480, 640), np.uint8)
    mask[60:420, 100:560] = 255
    m_dev = cuda.from_numpy(mask).cuda()
    with capi.Volume(cfg) as vol:
        if path == "default":
            for c2w, d in zip(poses, depths):
                vol.integrate(d, c2w)                               # deferred host frames
        elif path == "sequence":
            vol.integrate_frames_device([d.data_ptr() for d in d_dev], np.stack(poses))
        else:
            for c2w, d in zip(poses, d_dev):
                vol.integrate_masked_device(d.data_ptr(), m_dev.data_ptr(), c2w)
        for K, hw in RENDERS:
            for c2w in (scene.pose(16, n=64), scene.pose(19, n=64)):   # an integrated pose and one between two
                check_render(vol, params(K, hw), c2w, f"{dims} {path} {hw}")
        check_render(vol, params(K_OTHER, (97, 161), thr=2.5), poses[1], f"{dims} {path} thr 2.5")


def test_parity_labels_and_colour(cuda):
    dims = (160, 120, 132)
    cfg, vs, origin = volume_for(dims)
    scene, poses, depths = surf_frames(dims, vs, origin, range(0, 64, 16))
    rng = np.random.default_rng(3)
    with capi.Volume(cfg) as vol:
        vol.labels_enable(0.5)
        vol.colour_enable()
        for k, (c2w, d) in enumerate(zip(poses, depths)):
            d_dev = cuda.from_numpy(d).cuda()
            lab = cuda.from_numpy(rng.integers(1, 50, (480, 640)).astype(np.int16)).cuda()
            sc = cuda.from_numpy(rng.uniform(0.3, 1.0, (480, 640)).astype(f32)).cuda()
            rgb = cuda.from_numpy(rng.integers(0, 256, (480, 640, 3)).astype(np.uint8)).cuda()
            vol.integrate_device(d_dev.data_ptr(), c2w)
            vol.integrate_colour_device(d_dev.data_ptr(), rgb.data_ptr(), c2w)
            vol.integrate_labels_device(d_dev.data_ptr(), lab.data_ptr(), sc.data_ptr(), c2w)
            vol.sync()
        label = vol.download_labels()[0]
        colour = vol.download_colour()
        assert label.any() and colour.any()
        for K, hw in RENDERS:
            got, _ = check_render(vol, params(K, hw), scene.pose(5, n=64), f"labels {hw}", label=label, colour=colour)
        assert got["label"].dtype == np.uint16 and got["colour"].dtype == np.uint32


def edge_state(dims, rng):
    """A sphere's truncated SDF with NaN (payload), +-inf, +-0 values and weights at 0.9, one ulp above it, 0 and NaN."""
    dx, dy, dz = dims
    z, y, x = np.meshgrid(np.arange(dz), np.arange(dy), np.arange(dx), indexing="ij")
    c = np.array(dims) / 2.0
    sdf = np.sqrt((x - c[0]) ** 2 + (y - c[1]) ** 2 + (z - c[2]) ** 2) - 0.35 * min(dims)
    t = np.clip(sdf / 5.0, -1, 1).astype(f32).ravel()
    w = np.full(t.size, 3.0, f32)
    n = t.size
    idx = rng.choice(n, n // 50, replace=False)
    parts = np.array_split(idx, 9)
    t[parts[0]] = NAN_PAYLOAD
    t[parts[1]] = np.inf
    t[parts[2]] = -np.inf
    t[parts[3]] = -0.0
    t[parts[4]] = 0.0
    w[parts[5]] = f32(0.9)
    w[parts[6]] = np.nextafter(f32(0.9), f32(2))
    w[parts[7]] = 0.0
    w[parts[8]] = np.nan
    return t, w


@pytest.mark.parametrize("dims", [(128, 96, 64), (160, 120, 132)])
def test_parity_on_uploaded_value_edges(cuda, dims):
    rng = np.random.default_rng(11)
    cfg, vs, origin = volume_for(dims)
    t, w = edge_state(dims, rng)
    scene = synth.SurfScene(dims, vs, origin)
    with capi.Volume(cfg) as vol:
        vol.upload(t, w)
        for c2w in (scene.pose(3, n=64), synth.make_pose(np.eye(3), [0.0, 0.0, 0.9])):   # outside; inside the box
            for thr in (0.9, 0.0, -1.0):
                check_render(vol, params(synth.TUM_K, (480, 640), thr=thr), c2w, f"edges {dims} thr {thr}")


def subset_pixels(hw, stride=37):
    """Whole 8 x 8 tiles at the corners and the centre, plus a strided sample of the image."""
    h, w = hw
    px = set()
    for u0, v0 in ((0, 0), (w - 8, h - 8), (w // 2 - 4, h // 2 - 4), (w // 3, h // 3)):
        for dv in range(8):
            for du in range(8):
                px.add((u0 + du, v0 + dv))
    for v in range(0, h, stride // 3):
        for u in range(v % stride, w, stride):
            px.add((u, v))
    return np.array(sorted(px), np.int64)


def test_512_cubed_subset_parity_and_accuracy(cuda):
    E = 512
    cfg, vs, origin = volume_for((E, E, E), 0.0016)
    scene, poses, depths = surf_frames((E,) * 3, vs, origin, range(64))
    d_dev = [cuda.from_numpy(d).cuda() for d in depths]
    px = subset_pixels((480, 640))
    with capi.Volume(cfg) as vol:
        vol.integrate_frames_device([d.data_ptr() for d in d_dev], np.stack(poses))
        del d_dev
        for k in (8, 9):
            c2w = scene.pose(k, n=64)
            got, want = check_render(vol, params(synth.TUM_K, (480, 640)), c2w, f"512^3 k={k}", pixels=px)
            # the CPU test's accuracy bounds (tests/test_raycast_spec.py), on the sphere pixels of the subset
            z = scene.depth(c2w)[px[:, 1], px[:, 0]]
            T = np.asarray(c2w, np.float64).reshape(4, 4)
            dcam = np.stack([(px[:, 0] - synth.TUM_K[2]) / synth.TUM_K[0], (px[:, 1] - synth.TUM_K[5]) / synth.TUM_K[4],
                             np.ones(len(px))], -1)
            p_base = (dcam @ T[:3, :3].T) * z[:, None] + T[:3, 3]
            on_sphere = np.abs(np.linalg.norm(p_base - scene.center, axis=-1) - scene.radius) < 1e-6
            zz = scene.depth(c2w)
            from test_raycast_spec import SURF_MEDIAN_VS, SURF_P99_VS, away_from_edges
            m = on_sphere & away_from_edges(zz, vs)[px[:, 1], px[:, 0]]
            assert m.sum() > 100 and want["hit"][m].all()
            err = np.abs(want["depth"][m] - z[m]) / vs
            assert np.median(err) < SURF_MEDIAN_VS and np.percentile(err, 99) < SURF_P99_VS, (np.median(err), np.percentile(err, 99))


# ------------------------------------------------------------------------------------------------------------------------
# ordering and read-only
# ------------------------------------------------------------------------------------------------------------------------
def test_deferred_frames_are_applied_before_a_render(cuda):
    dims = (128, 96, 64)
    cfg, vs, origin = volume_for(dims)
    scene, poses, depths = surf_frames(dims, vs, origin, range(0, 40, 8))
    p = params(synth.TUM_K, (480, 640))
    view = scene.pose(4, n=64)
    with capi.Volume(cfg) as a, capi.Volume(cfg) as b:
        for c2w, d in zip(poses, depths):
            a.integrate(d, c2w)                                     # five collected host frames, no sync
        ra = a.raycast(view, params=p)
        b.set_deferral(0)
        for c2w, d in zip(poses, depths):
            b.integrate(d, c2w)
        rb = b.raycast(view, params=p)
        assert (ra["depth"] > 0).sum() > 1000
        same_bits(ra["depth"], rb["depth"], "deferred depth")
        same_bits(ra["normal"], rb["normal"], "deferred normal")


def test_render_on_a_caller_stream_and_host_device_equality(cuda):
    dims = (128, 96, 64)
    cfg, vs, origin = volume_for(dims)
    scene, poses, depths = surf_frames(dims, vs, origin, range(0, 64, 16))
    p = params(K_OTHER, (97, 161))
    view = scene.pose(6, n=64)
    with capi.Volume(cfg) as vol:
        s = cuda.cuda.Stream()
        vol.set_stream(s.cuda_stream)
        host_d = [cuda.from_numpy(d).pin_memory() for d in depths]
        with cuda.cuda.stream(s):
            dev = [x.to("cuda", non_blocking=True) * 1.0 for x in host_d]   # produced by work queued on s
            for c2w, d in zip(poses, dev):
                vol.integrate_device(d.data_ptr(), c2w)
            depth = cuda.empty((97, 161), dtype=cuda.float32, device="cuda")
            normal = cuda.empty((97, 161, 3), dtype=cuda.float32, device="cuda")
            depth.fill_(-7.0)
            vol.raycast_device(view, depth.data_ptr(), normal.data_ptr(), params=p)
        s.synchronize()
        got = vol.raycast(view, params=p)
        same_bits(depth.cpu().numpy(), got["depth"], "device vs host depth")
        same_bits(normal.cpu().numpy(), got["normal"], "device vs host normal")
        assert (got["depth"] > 0).sum() > 100
        vol.set_stream(None)
        check_render(vol, p, view, "after stream")


def test_render_reads_only(cuda):
    dims = (128, 96, 64)
    cfg, vs, origin = volume_for(dims)
    scene, poses, depths = surf_frames(dims, vs, origin, range(0, 64, 16))
    with capi.Volume(cfg) as vol:
        vol.labels_enable(0.5)
        vol.colour_enable()
        lab = cuda.full((480, 640), 3, dtype=cuda.int16, device="cuda")
        sc = cuda.full((480, 640), 0.8, dtype=cuda.float32, device="cuda")
        rgb = cuda.full((480, 640, 3), 90, dtype=cuda.uint8, device="cuda")
        for c2w, d in zip(poses, depths):
            dd = cuda.from_numpy(d).cuda()
            vol.integrate_device(dd.data_ptr(), c2w)
            vol.integrate_colour_device(dd.data_ptr(), rgb.data_ptr(), c2w)
            vol.integrate_labels_device(dd.data_ptr(), lab.data_ptr(), sc.data_ptr(), c2w)
        before = (*vol.download(), *vol.download_labels(), vol.download_colour())
        for k in range(3):
            vol.raycast(scene.pose(k * 5, n=64), params=params(synth.TUM_K, (480, 640)), labels=True, colour=True)
        after = (*vol.download(), *vol.download_labels(), vol.download_colour())
        for x, y, name in zip(before, after, ("tsdf", "weight", "label", "fp", "bp", "colour")):
            assert x.tobytes() == y.tobytes(), name
        assert vol.count_surface() > 0


# ------------------------------------------------------------------------------------------------------------------------
# batch
# ------------------------------------------------------------------------------------------------------------------------
def batch_cfgs(n, E, overlapping=False):
    """tools/batch_time.py's members: n boxes of E^3 voxels at 0.8 / E m with random origins (two coincident boxes when
    overlapping), and a {0, 255} instance mask each."""
    rng = np.random.default_rng(0)
    vs = 0.8 / E
    K = synth.TUM_K
    cfgs, masks = [], []
    for i in range(n):
        o = np.array([-0.4 + rng.uniform(-0.3, 0.3), -0.4 + rng.uniform(-0.25, 0.25), 0.7 + rng.uniform(0, 0.8)], f32)
        if overlapping and i == 1:
            o = cfgs[0].origin[:]
            o = np.array(o, f32) + np.array([0.1, 0.05, 0.1], f32)
        cfgs.append(capi.make_config((E, E, E), vs, o, vol_id=i))
        m = np.zeros((480, 640), np.uint8)
        c = o + 0.4
        u0, u1 = K[0] * (c[0] - 0.25) / c[2] + K[2], K[0] * (c[0] + 0.25) / c[2] + K[2]
        v0, v1 = K[4] * (c[1] - 0.25) / c[2] + K[5], K[4] * (c[1] + 0.25) / c[2] + K[5]
        m[max(0, int(v0)):max(0, min(480, int(v1))), max(0, int(u0)):max(0, min(640, int(u1)))] = 255
        masks.append(m)
    return cfgs, masks


@pytest.mark.parametrize("n, E, overlapping", [(16, 200, False), (2, 128, True)], ids=["16x200", "overlap"])
def test_batch_is_the_nearest_member(cuda, n, E, overlapping):
    cfgs, masks = batch_cfgs(n, E, overlapping)
    scene = synth.SurfScene((200, 200, 200), 0.004, np.array([-0.4, -0.4, 0.7], f32))
    poses = [scene.pose(k, 8) for k in range(8)]
    depth = cuda.from_numpy(scene.depth(poses[0])).cuda()
    m_dev = [cuda.from_numpy(m).cuda() for m in masks]
    p = params(synth.TUM_K, (480, 640))
    view = scene.pose(3, 8)
    with capi.Batch(cfgs) as batch:
        for k in range(12):                                         # collected, then applied by the render's flush
            batch.integrate_device(depth.data_ptr(), [m.data_ptr() for m in m_dev], poses[k % 8])
        d = cuda.empty((480, 640), dtype=cuda.float32, device="cuda")
        nrm = cuda.empty((480, 640, 3), dtype=cuda.float32, device="cuda")
        who = cuda.empty((480, 640), dtype=cuda.int32, device="cuda")
        batch.raycast_device(view, d.data_ptr(), nrm.data_ptr(), who.data_ptr(), params=p)
        batch.sync()
        got = (d.cpu().numpy(), nrm.cpu().numpy(), who.cpu().numpy())
        singles = [v.raycast(view, params=p) for v in batch.volumes]
    dd = np.stack([np.where(s["depth"] > 0, s["depth"], np.inf) for s in singles])
    best = np.argmin(dd, axis=0)
    anyhit = np.isfinite(dd.min(axis=0))
    want_who = np.where(anyhit, best, -1).astype(np.int32)
    ii, jj = np.meshgrid(np.arange(480), np.arange(640), indexing="ij")
    want_d = np.where(anyhit, dd[best, ii, jj], 0).astype(f32)
    want_n = np.where(anyhit[..., None], np.stack([s["normal"] for s in singles])[best, ii, jj], 0).astype(f32)
    assert anyhit.sum() > 2000 and len(np.unique(want_who)) > min(n, 3)
    same_bits(got[2], want_who, "member")
    same_bits(got[0], want_d, "depth")
    same_bits(got[1], want_n, "normal")
    if overlapping:
        both = np.all(np.isfinite(dd), axis=0)
        assert both.sum() > 100                                       # pixels where both members have a hit


# ------------------------------------------------------------------------------------------------------------------------
# refusals
# ------------------------------------------------------------------------------------------------------------------------
def test_refusals(cuda):
    lib = capi.load()
    eye = np.eye(4, dtype=f32).ravel()
    buf = cuda.empty(480 * 640 * 3, dtype=cuda.float32, device="cuda")
    ptr = buf.data_ptr()

    def refused(vol_h, p, what, depth=ptr, normal=None, label=None, colour=None):
        rc = lib.tsdf_raycast_device(vol_h, C.byref(p), eye.ctypes.data, depth, normal, label, colour)
        msg = lib.tsdf_last_error().decode()
        assert rc == -1 and what in msg, (rc, msg)

    cfg = capi.make_config((64, 32, 16), 0.01, [0, 0, 0.5])
    with capi.Volume(cfg) as vol:
        good = capi.raycast_params_default(cfg)
        refused(vol._h, good, "tsdf_labels_enable", depth=None, label=ptr)
        refused(vol._h, good, "tsdf_colour_enable", depth=None, colour=ptr)
        refused(vol._h, good, "every output is NULL", depth=None)
        for field, value, what in (("near_m", -0.1, "near"), ("far_m", float("inf"), "near"), ("near_m", 6.0, "near"),
                                   ("im_height", 0, "image size"), ("im_width", -3, "image size")):
            p = capi.raycast_params_default(cfg)
            setattr(p, field, value)
            refused(vol._h, p, what)
        for i, value, what in ((0, 0.0, "fx and fy"), (4, 0.0, "fx and fy"), (2, float("nan"), "cam_K[2]"),
                               (0, float("inf"), "cam_K[0]")):
            p = capi.raycast_params_default(cfg)
            p.cam_K[i] = value
            refused(vol._h, p, what)
        vol.raycast(eye, params=good)                                  # and a good call still works
    with capi.Volume(capi.make_config((64, 32, 16), 0.01, [0, 0, 0.5], z_begin=4, z_end=12)) as slab:
        refused(slab._h, good, "z-slab")
    with capi.Volume(capi.make_config((64, 1, 16), 0.01, [0, 0, 0.5])) as flat:
        refused(flat._h, good, "dim must be >= 2")
    with capi.Batch([capi.make_config((64, 32, 16), 0.01, [0, 0, 0.5]), capi.make_config((64, 32, 1), 0.01, [0, 0, 0.5])]) as b:
        rc = lib.tsdf_batch_raycast_device(b._h, C.byref(good), eye.ctypes.data, ptr, None, None)
        assert rc == -1 and "dim must be >= 2" in lib.tsdf_last_error().decode()
        rc = lib.tsdf_batch_raycast_device(b._h, C.byref(good), eye.ctypes.data, None, None, None)
        assert rc == -1 and "every output is NULL" in lib.tsdf_last_error().decode()
