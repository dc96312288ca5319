"""Tracking on the device (tsdf_track / tsdf_track_system, csrc/tsdf_track.hip.h) against its float32 restatement
(tests/track_spec.py): the system of one iteration term by term over levels, masks, grid shapes and image sizes (the spec fed
the device's own render, which is bit-exact with raycast_spec; each entry within n * 2^-52 * sum |term|, what two double sums of
the same n terms can differ by); convergence on a 256^3 volume within the CPU bounds and every entry of the pose within one
float32 ulp of the spec's track from the same render; a stretch of the fr3 trajectory; an object of a batch;
determinism, read-only-ness, ordering and the refusals of the C ABI."""
import ctypes as C
import math
import os

import numpy as np
import pytest

import track_cases as tc
import track_spec as ts
from semantic_slam_amd import capi, synth, ingest

pytestmark = pytest.mark.gpu

f32 = np.float32
EYE = np.eye(4, dtype=f32).ravel()
COS_WIDE = math.cos(math.radians(40.0))       # test_track_spec.py: the angle 3 deg / 3 cm guesses need


def scaled(K, by):
    K = np.asarray(K, np.float64).copy()
    K[[0, 2, 4, 5]] /= by
    return K.astype(f32)


def track_params(cfg, K, hw, cos_thresh=None, **kw):
    p = capi.track_params_default(cfg)
    p.ray.cam_K[:] = [float(x) for x in np.asarray(K, f32).ravel()]
    p.ray.im_height, p.ray.im_width = hw
    if cos_thresh is not None:
        p.cos_normal_thresh = cos_thresh
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def fused_volume(cuda, dims, vs, z0=0.8, poses_k=range(0, 64, 2), base2world=None):
    """A TrackScene volume fused on the device from 640 x 480 TUM frames of the orbit."""
    origin = synth.surf_volume(max(dims), vs, z0)
    cfg = capi.make_config(dims, vs, origin, base2world=base2world)
    scene = synth.TrackScene(dims, vs, origin)
    poses = [scene.pose(k) for k in poses_k]
    frames = [cuda.from_numpy(scene.depth(c, quantize=True)).cuda() for c in poses]
    vol = capi.Volume(cfg)
    vol.integrate_frames_device([d.data_ptr() for d in frames], np.stack(poses))
    vol.sync()
    return vol, cfg, origin


def device_model(vol, p, pose):
    """The device's render at pose with p.ray (bit-exact with raycast_spec, test_gpu_raycast.py)."""
    o = vol.raycast(pose, params=p.ray, normals=True)
    return o["depth"], o["normal"]


def c2b(cfg, c2w):
    return capi.multiply_matrix(capi.invert_matrix(np.asarray(cfg.base2world, f32))[1], c2w)


def check_system(vol, cfg, p, live, mask, ref, cur, level, what):
    d_dev = live_dev(live)
    m_dev = None if mask is None else mask_dev(mask)
    A, b, r2, n = vol.track_system(d_dev.data_ptr(), ref, cur, level=level, params=p,
                                   mask_ptr=None if m_dev is None else m_dev.data_ptr())
    got = np.concatenate([A[np.triu_indices(6)], b, [r2, n]])
    want, absum = ts.system((live, mask), device_model(vol, p, ref), level, ts.relative(c2b(cfg, ref), c2b(cfg, cur)),
                            ts.from_ctypes(p))
    assert n == want[28], f"{what}: {n} pairs, spec {want[28]}"
    assert n > 50, what
    bad = np.abs(got - want) > n * 2.0 ** -52 * absum             # two double sums of the same n float32 terms
    assert not bad.any(), f"{what}: entries {np.nonzero(bad)[0].tolist()} differ: {got[bad]} vs {want[bad]}"
    return n


_torch = None


def live_dev(depth):
    return _torch.from_numpy(np.ascontiguousarray(depth, f32)).cuda()


def mask_dev(mask):
    return _torch.from_numpy(np.ascontiguousarray(mask, np.uint8)).cuda()


@pytest.fixture(autouse=True)
def _bind_torch(cuda):
    global _torch
    _torch = cuda


# ------------------------------------------------------------------------------------------------------------------------
# the system, term by term
# ------------------------------------------------------------------------------------------------------------------------
K_OTHER = np.array([300.0, 0, 75.3, 0, 310.0, 52.1, 0, 0, 1], f32)


@pytest.mark.parametrize("dims", [(128, 96, 80), (160, 120, 132)])
@pytest.mark.parametrize("K, hw", [(synth.TUM_K, (480, 640)), (K_OTHER, (97, 161)), (scaled(synth.TUM_K, 2), (237, 331))],
                         ids=["640x480", "161x97", "331x237"])
def test_system_parity(cuda, dims, K, hw):
    vs = 0.768 / max(dims)
    vol, cfg, origin = fused_volume(cuda, dims, vs, poses_k=range(0, 64, 8))
    with vol:
        scene = synth.TrackScene(dims, vs, origin, K=K, h=hw[0], w=hw[1])
        p = track_params(cfg, K, hw, cos_thresh=COS_WIDE)
        true = scene.pose(9)
        ref = ts.perturb(true, np.random.default_rng(4), 2.0, 0.02)
        live = scene.depth(true, quantize=True)
        mask = np.zeros(hw, np.uint8)
        mask[hw[0] // 6: hw[0] - hw[0] // 5, hw[1] // 7: hw[1] - hw[1] // 4] = 255
        mask[::5, ::3] = 127                                      # just below the threshold
        for level in range(3):
            for m in (None, mask):
                check_system(vol, cfg, p, live, m, ref, true, level, f"{dims} {hw} level {level} mask {m is not None}")
        # at the reference pose itself (M = identity) and with a base pose
        check_system(vol, cfg, p, live, None, true, true, 0, "ref = cur")


def test_system_parity_with_a_base_pose(cuda):
    dims, vs = (128, 96, 80), 0.006
    base = synth.make_pose(synth.rot_y(0.2) @ synth.rot_x(-0.1), [0.3, -0.2, 0.1])
    origin = synth.surf_volume(max(dims), vs, 0.8)
    cfg = capi.make_config(dims, vs, origin, base2world=base)
    scene = synth.TrackScene(dims, vs, origin)
    with capi.Volume(cfg) as vol:
        for k in range(0, 64, 8):
            c = scene.pose(k)
            vol.integrate(scene.depth(c, quantize=True), capi.multiply_matrix(base, c))    # cam2world = base * cam2base
        p = track_params(cfg, synth.TUM_K, (480, 640), cos_thresh=COS_WIDE)
        true = capi.multiply_matrix(base, scene.pose(9))
        ref = capi.multiply_matrix(base, ts.perturb(scene.pose(9), np.random.default_rng(2), 2.0, 0.02))
        live = scene.depth(scene.pose(9), quantize=True)
        for level in range(3):
            check_system(vol, cfg, p, live, None, ref, true, level, f"base level {level}")


# ------------------------------------------------------------------------------------------------------------------------
# convergence (test_track_spec.py's held-out poses, perturbations and bounds)
# ------------------------------------------------------------------------------------------------------------------------
HELD_OUT = (5, 13, 27, 41, 55)
FUSED_M, FUSED_RAD = 1.2e-3, 8e-4            # test_track_spec.py


def check_spec_pose(got, want, what):
    """Every entry of the float32 pose within one float32 ulp of the restatement's (test_gpu_track_exact.py)."""
    u = tc.ulps32(np.asarray(got, f32).ravel(), want)
    assert u.max() <= 1.0, f"{what}: entries {np.nonzero(u > 1.0)[0].tolist()} off by {u[u > 1.0]} float32 ulps"


@pytest.fixture(scope="module")
def vol256(cuda):
    vol, cfg, origin = fused_volume(cuda, (256,) * 3, 0.003)
    yield vol, cfg, origin
    vol.close()


def test_convergence_matches_the_cpu_bounds_and_the_spec(vol256):
    vol, cfg, origin = vol256
    K, hw = scaled(synth.TUM_K, 2), (240, 320)
    scene = synth.TrackScene(cfg_dims(cfg), 0.003, origin, K=K, h=hw[0], w=hw[1])
    p = track_params(cfg, K, hw, cos_thresh=COS_WIDE)
    P = ts.from_ctypes(p)
    rng = np.random.default_rng(1)
    errs = []
    for k in HELD_OUT:
        true = scene.pose(k)
        guess = ts.perturb(true, rng)
        live = scene.depth(true, quantize=True)
        d = live_dev(live)
        got, st = vol.track(d.data_ptr(), guess, params=p)
        assert st["status"] != 2, (k, st)
        errs.append(ts.pose_error(got, true))
        spec = ts.track((live, None), device_model(vol, p, guess), P)
        want = ts.result_pose(np.asarray(cfg.base2world, f32), c2b(cfg, guess), spec["M"])
        check_spec_pose(got, want, (k, st, spec))
        assert (st["status"], st["iters_run"], st["inliers"]) == (spec["status"], spec["iters_run"], spec["inliers"]), (k, st, spec)
    errs = np.array(errs)
    print(f"256^3: worst {errs[:, 0].max():.2e} m, {errs[:, 1].max():.2e} rad")
    assert errs[:, 0].max() < FUSED_M and errs[:, 1].max() < FUSED_RAD, errs


def cfg_dims(cfg):
    return (cfg.dim_x, cfg.dim_y, cfg.dim_z)


def test_determinism_and_read_only(vol256, cuda):
    vol, cfg, origin = vol256
    scene = synth.TrackScene(cfg_dims(cfg), 0.003, origin)
    true = scene.pose(21)
    guess = ts.perturb(true, np.random.default_rng(3), 1.0, 0.01)
    d = live_dev(scene.depth(true, quantize=True))
    before = vol.download()
    a = vol.track(d.data_ptr(), guess)
    b = vol.track(d.data_ptr(), guess)
    A1 = vol.track_system(d.data_ptr(), guess, true, level=1)
    A2 = vol.track_system(d.data_ptr(), guess, true, level=1)
    after = vol.download()
    assert a[0].tobytes() == b[0].tobytes() and a[1] == b[1]
    assert all(np.asarray(x).tobytes() == np.asarray(y).tobytes() for x, y in zip(A1, A2))
    assert a[1]["status"] == 0, a[1]                                # 1 deg / 1 cm at the default parameters
    for x, y, name in zip(before, after, ("tsdf", "weight")):
        assert x.tobytes() == y.tobytes(), name


# ------------------------------------------------------------------------------------------------------------------------
# a stretch of the fr3 trajectory
# ------------------------------------------------------------------------------------------------------------------------
def interp(T0, T1, a):
    T0 = np.asarray(T0, np.float64).reshape(4, 4)
    T1 = np.asarray(T1, np.float64).reshape(4, 4)
    dR = T0[:3, :3].T @ T1[:3, :3]
    sn = 0.5 * np.array([dR[2, 1] - dR[1, 2], dR[0, 2] - dR[2, 0], dR[1, 0] - dR[0, 1]])
    ang = math.atan2(np.linalg.norm(sn), (np.trace(dR) - 1) / 2)
    w = sn / np.linalg.norm(sn) * ang if ang > 0 else np.zeros(3)
    T = np.eye(4)
    T[:3, :3] = T0[:3, :3] @ ts.rodrigues(a * w)
    T[:3, 3] = (1 - a) * T0[:3, 3] + a * T1[:3, 3]
    return T.astype(f32).ravel()


TRAJ = range(0, 8)        # keyframes fused (0.7 m sideways, 10 deg from the base); tracked between 0 and 6 at 1/8 steps
# Every step must agree with the restatement run on the device's own render (check_spec_pose), so the drift is the
# restatement's; measured over the 48 steps: worst 1.65e-4 m, 8.1e-5 rad.  The bounds are about 3x and 4x that.
TRAJ_M, TRAJ_RAD = 5e-4, 3e-4


def test_trajectory_drift(cuda):
    gold = np.load(ingest_golden(), allow_pickle=False)
    Twc = ingest.pose_inverse(gold["Tcw"])
    base = Twc[0].ravel().astype(f32)
    dims, vs = (256, 256, 256), 0.008
    half = dims[0] * vs / 2.0
    origin = np.array([-half, -half, 0.6], f32)
    cfg = capi.make_config(dims, vs, origin, base2world=base)
    scene = synth.TrackScene(dims, vs, origin)
    binv = capi.invert_matrix(base)[1]
    poses = [Twc[i].ravel().astype(f32) for i in TRAJ]
    frames = [live_dev(scene.depth(capi.multiply_matrix(binv, c), quantize=True)) for c in poses]
    p = capi.track_params_default(cfg)
    P = ts.from_ctypes(p)
    with capi.Volume(cfg) as vol:
        vol.integrate_frames_device([d.data_ptr() for d in frames], np.stack(poses))
        est = poses[0]
        worst = (0.0, 0.0)
        for kf in range(6):
            for j in range(1, 9):
                true = interp(poses[kf], poses[kf + 1], j / 8.0)
                live = scene.depth(capi.multiply_matrix(binv, true), quantize=True)
                got, st = vol.track(live_dev(live).data_ptr(), est, params=p)
                assert st["status"] != 2, (kf, j, st)
                spec = ts.track((live, None), device_model(vol, p, est), P)
                want = ts.result_pose(base, c2b(cfg, est), spec["M"])
                check_spec_pose(got, want, (kf, j))
                est = got
                d = ts.pose_error(est, true)
                worst = (max(worst[0], d[0]), max(worst[1], d[1]))
        print(f"trajectory: worst drift {worst[0]:.2e} m, {worst[1]:.2e} rad")
        assert worst[0] < TRAJ_M and worst[1] < TRAJ_RAD, worst


def ingest_golden():
    return os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fr3_office_keyframes.npz")


# ------------------------------------------------------------------------------------------------------------------------
# an object of a batch
# ------------------------------------------------------------------------------------------------------------------------
def test_object_tracking_on_a_batch_member(cuda):
    dims, vs = (200, 200, 200), 0.768 / 200
    origin = synth.surf_volume(200, vs, 0.8)
    scene = synth.TrackScene(dims, vs, origin)
    other = capi.make_config((64, 64, 64), 0.01, [-0.3, -0.3, 2.5], vol_id=1)
    cfgs = [capi.make_config(dims, vs, origin, vol_id=0), other]
    poses = [scene.pose(k) for k in range(0, 64, 4)]
    mask = np.zeros((480, 640), np.uint8)
    mask[90:400, 120:540] = 255                                   # both spheres and the wall between them
    m = mask_dev(mask)
    with capi.Batch(cfgs) as batch:
        for c in poses:
            d = live_dev(scene.depth(c, quantize=True))
            batch.integrate_device(d.data_ptr(), [m.data_ptr(), None], c)   # collected; the track applies them first
        vol = batch.volumes[0]
        p = track_params(cfgs[0], synth.TUM_K, (480, 640))
        true = scene.pose(7)
        guess = ts.perturb(true, np.random.default_rng(5), 1.0, 0.01)
        live = scene.depth(true, quantize=True)
        got, st = vol.track(live_dev(live).data_ptr(), guess, params=p, mask_ptr=m.data_ptr())
        assert st["status"] == 0, st
        spec = ts.track((live, mask), device_model(vol, p, guess), ts.from_ctypes(p))
        want = ts.result_pose(EYE, guess, spec["M"])
        check_spec_pose(got, want, "batch member")
        e = ts.pose_error(got, true)
        assert e[0] < FUSED_M and e[1] < FUSED_RAD, e
        check_system(vol, cfgs[0], p, live, mask, guess, true, 0, "batch member")


# ------------------------------------------------------------------------------------------------------------------------
# ordering
# ------------------------------------------------------------------------------------------------------------------------
def test_deferred_frames_and_caller_stream_order_the_call(cuda):
    dims, vs = (128, 96, 80), 0.006
    origin = synth.surf_volume(128, vs, 0.8)
    cfg = capi.make_config(dims, vs, origin)
    scene = synth.TrackScene(dims, vs, origin)
    poses = [scene.pose(k) for k in range(0, 64, 8)]
    depths = [scene.depth(c, quantize=True) for c in poses]
    true = scene.pose(9)
    guess = ts.perturb(true, np.random.default_rng(6), 1.0, 0.01)
    live = live_dev(scene.depth(true, quantize=True))
    with capi.Volume(cfg) as ref:
        ref.set_deferral(0)
        for c, d in zip(poses, depths):
            ref.integrate(d, c)
        want = ref.track(live.data_ptr(), guess)
    assert want[1]["status"] != 2
    with capi.Volume(cfg) as a:                                   # collected host frames, no sync
        for c, d in zip(poses, depths):
            a.integrate(d, c)
        got = a.track(live.data_ptr(), guess)
    assert got[0].tobytes() == want[0].tobytes() and got[1] == want[1]
    with capi.Volume(cfg) as b:
        s = cuda.cuda.Stream()
        b.set_stream(s.cuda_stream)
        host = [cuda.from_numpy(d).pin_memory() for d in depths]
        with cuda.cuda.stream(s):
            dev = [x.to("cuda", non_blocking=True) * 1.0 for x in host]     # produced by work queued on s
            for c, d in zip(poses, dev):
                b.integrate_device(d.data_ptr(), c)
            lv = live * 1.0
            got = b.track(lv.data_ptr(), guess)
        b.set_stream(None)
    assert got[0].tobytes() == want[0].tobytes() and got[1] == want[1]


# ------------------------------------------------------------------------------------------------------------------------
# lost and refusals
# ------------------------------------------------------------------------------------------------------------------------
def test_lost_returns_the_guess(cuda):
    cfg = capi.make_config((64, 64, 64), 0.01, [-0.32, -0.32, 0.8])
    guess = synth.make_pose(synth.rot_y(0.1), [0.01, 0.02, -0.03])
    scene = synth.TrackScene((64, 64, 64), 0.01, [-0.32, -0.32, 0.8])
    with capi.Volume(cfg) as vol:
        got, st = vol.track(live_dev(scene.depth(guess)).data_ptr(), guess)          # an empty volume
        assert st["status"] == 2 and st["inliers"] == 0 and got.tobytes() == guess.tobytes()
        vol.integrate(scene.depth(guess, quantize=True), guess)
        got, st = vol.track(live_dev(np.zeros((480, 640), f32)).data_ptr(), guess)   # an all-zero frame
        assert st["status"] == 2 and got.tobytes() == guess.tobytes()
        assert st["iters_run"] == [0, 0, 1]


def test_refusals(cuda):
    lib = capi.load()
    buf = cuda.zeros(480 * 640, dtype=cuda.float32, device="cuda")
    ptr = buf.data_ptr()
    res = capi.TrackResult()
    sysbuf = np.zeros(29)

    def refused(h, p, what, depth=ptr, out=True, level=0, system=False):
        if system:
            rc = lib.tsdf_track_system(h, C.byref(p), depth, None, EYE.ctypes.data, EYE.ctypes.data, level,
                                       sysbuf.ctypes.data if out else None)
        else:
            rc = lib.tsdf_track(h, C.byref(p), depth, None, EYE.ctypes.data, C.byref(res) if out else None)
        msg = lib.tsdf_last_error().decode()
        assert rc == -1 and what in msg, (rc, msg)

    cfg = capi.make_config((64, 32, 16), 0.01, [0, 0, 0.5])
    with capi.Volume(cfg) as vol:
        good = capi.track_params_default(cfg)
        for system in (False, True):
            refused(vol._h, good, "NULL depth", depth=None, system=system)
            refused(vol._h, good, "NULL result", out=False, system=system)
            for field, value, what in (("n_levels", 0, "n_levels"), ("n_levels", 4, "n_levels"),
                                       ("cos_normal_thresh", 1.5, "cos_normal_thresh"),
                                       ("cos_normal_thresh", -1.01, "cos_normal_thresh"),
                                       ("cos_normal_thresh", float("nan"), "cos_normal_thresh"),
                                       ("eps_rot", 0.0, "eps_rot"), ("eps_trans", float("inf"), "eps_rot"),
                                       ("min_inliers", -1, "min_inliers")):
                p = capi.track_params_default(cfg)
                setattr(p, field, value)
                refused(vol._h, p, what, system=system)
            for arr, i, value, what in (("iters", 2, -1, "iters[2]"), ("dist_thresh", 0, 0.0, "dist_thresh[0]"),
                                        ("dist_thresh", 1, float("nan"), "dist_thresh[1]"),
                                        ("dist_thresh", 2, -0.1, "dist_thresh[2]")):
                p = capi.track_params_default(cfg)
                getattr(p, arr)[i] = value
                refused(vol._h, p, what, system=system)
            p = capi.track_params_default(cfg)
            p.ray.near_m = -1.0
            refused(vol._h, p, "near", system=system)
        p = capi.track_params_default(cfg)
        p.n_levels = 2
        refused(vol._h, p, "level 2 is outside", level=2, system=True)
        refused(vol._h, p, "level -1 is outside", level=-1, system=True)
        vol.track(ptr, EYE)                                          # and a good call still works
    with capi.Volume(capi.make_config((64, 32, 16), 0.01, [0, 0, 0.5], z_begin=4, z_end=12)) as slab:
        refused(slab._h, good, "z-slab")
    g = C.c_void_p()
    devs = (C.c_int32 * 1)(0)
    assert lib.tsdf_group_create(C.byref(cfg), devs, 1, C.byref(g)) == 0
    try:
        h = C.c_void_p()
        assert lib.tsdf_group_volume(g, 0, C.byref(h)) == 0
        refused(h, good, "tsdf_group")
    finally:
        lib.tsdf_group_destroy(g)
