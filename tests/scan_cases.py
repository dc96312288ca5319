"""The named lidar cases (test infrastructure, no GPU): the smallest inputs at which the kernels of csrc/tsdf_scan.hip.h can go
wrong.  Each case is built once, asserts here, on the CPU, that the restatement (tests/scan_spec.py) reaches the branch it is
named for, and carries the restatement's images; tests/test_scan_spec.py runs the assertions, tests/test_gpu_scan.py holds the
device to the images bit for bit."""
import functools
import os

import numpy as np

import scan_spec as spec
from semantic_slam_amd import synth

F = np.float32
H, W = 45, 61                       # odd in both directions, and no multiple of a 16 x 16 tile
K_SMALL = np.array([50.0, 0.0, 30.0, 0.0, 40.0, 22.0, 0.0, 0.0, 1.0], F)     # principal point ON pixel (30, 22)
# h = (x, y, z): uf = x / z, vf = y / z with nothing rounded on the way to h
M_PLAIN = np.array([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0]], F)
# h = (x + 4, y + 2, z + 1): the all-zero point lands at pixel (4, 2)
M_SHIFT = np.array([[1, 0, 0, 4], [0, 1, 0, 2], [0, 0, 1, 1]], F)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "kitti_2011_09_30_calib.npz")
KITTI_H, KITTI_W = 375, 1242

up = lambda a: np.nextafter(F(a), F(np.inf))          # noqa: E731
down = lambda a: np.nextafter(F(a), F(-np.inf))       # noqa: E731


def _pts(rows):
    """[n, 4] points from (x, y, z) rows, with an intensity nothing reads."""
    xyz = np.asarray(rows, F).reshape(-1, 3)
    return np.ascontiguousarray(np.concatenate([xyz, np.full((len(xyz), 1), 0.5, F)], axis=1))


def _case(name, points, velo2img, K=K_SMALL, h=H, w=W):
    points = np.ascontiguousarray(points, dtype=F).reshape(-1, 4)
    full = spec.project_full(points, velo2img, h, w)
    return {"name": name, "points": points, "velo2img": np.asarray(velo2img, F), "K": np.asarray(K, F), "H": h, "W": w,
            "full": full, "range": full["range"], "n_pixels": full["n_pixels"], "depth": spec.range_to_depth(full["range"], K)}


# ---- point counts -------------------------------------------------------------------------------------------------
def _count_case(n):
    rng = np.random.default_rng(100 + n)
    z = rng.uniform(1.0, 5.0, n)
    uf = rng.uniform(-5.0, W + 9.0, n)
    vf = rng.uniform(-5.0, H + 5.0, n)
    if n:
        uf[0], vf[0], z[0] = 10.5, 7.5, 2.0             # one point that is certainly written
    c = _case(f"count_{n}", _pts(np.stack([uf * z, vf * z, z], axis=1)), M_PLAIN)
    reason = c["full"]["reason"]
    assert len(reason) == n
    if n == 0:
        assert c["n_pixels"] == 0 and not c["range"].any()
    else:
        assert reason[0] == spec.ACCEPTED and c["range"][7, 10] > 0
        assert c["n_pixels"] >= 1
    if n >= 63:
        assert np.count_nonzero(reason == spec.ACCEPTED) > 20 and np.count_nonzero(reason != spec.ACCEPTED) > 5
    if n == 4097:      # more accepted points than written pixels: collisions, across wavefronts and workgroups
        assert np.count_nonzero(reason == spec.ACCEPTED) > c["n_pixels"] > 1000
    return c


# ---- collisions ---------------------------------------------------------------------------------------------------
def _one_pixel(scales):
    """Points along the ray of pixel (10, 7), one per scale: all land there, each with a range of its own."""
    s = np.asarray(scales, np.float64)
    return _pts(np.stack([10.5 * s, 7.5 * s, s], axis=1))


def _collision_cases():
    out = []
    s = 1.0 + np.arange(1000) / 500.0
    c = _case("collide_1000_in_order", _one_pixel(s), M_PLAIN)
    f = c["full"]
    rng_of = np.sqrt((c["points"][:, 0] ** 2 + c["points"][:, 1] ** 2) + c["points"][:, 2] ** 2)
    assert np.all(f["reason"] == spec.ACCEPTED) and np.all(f["u"] == 10) and np.all(f["v"] == 7)
    assert len(np.unique(rng_of)) == 1000 and c["n_pixels"] == 1
    assert f["winner"][7, 10] == 999 and c["range"][7, 10] == rng_of[999]
    out.append(c)
    perm = np.concatenate([[999], np.random.default_rng(7).permutation(999)])      # the largest range first
    c = _case("collide_1000_permuted", _one_pixel(s[perm]), M_PLAIN)
    f = c["full"]
    rng_of = np.sqrt((c["points"][:, 0] ** 2 + c["points"][:, 1] ** 2) + c["points"][:, 2] ** 2)
    assert np.all(f["reason"] == spec.ACCEPTED) and c["n_pixels"] == 1
    assert np.argmax(rng_of) == 0 and f["winner"][7, 10] == 999
    assert c["range"][7, 10] == rng_of[999] < rng_of.max()           # the index decides, not the range
    out.append(c)
    # two pairs among points that are all rejected: 64 apart (one wavefront's width) and 4096 apart (other workgroups);
    # in each pair the EARLIER point has the larger range
    pts = np.zeros((4300, 3))
    pts[:, 2] = 1.0                                                    # h0 = 0: below the guard
    pts[5] = np.array([10.5, 7.5, 1.0]) * 3.0
    pts[5 + 64] = np.array([10.5, 7.5, 1.0]) * 2.0
    pts[100] = np.array([20.5, 30.5, 1.0]) * 3.0
    pts[100 + 4096] = np.array([20.5, 30.5, 1.0]) * 2.0
    c = _case("collide_64_and_4096_apart", _pts(pts), M_PLAIN)
    f = c["full"]
    assert np.count_nonzero(f["reason"] == spec.ACCEPTED) == 4 and np.count_nonzero(f["reason"] == spec.BELOW_GUARD) == 4296
    assert c["n_pixels"] == 2 and f["winner"][7, 10] == 69 and f["winner"][30, 20] == 4196
    assert c["range"][7, 10] < np.sqrt(F(31.5) ** 2 + F(22.5) ** 2 + F(9))
    out.append(c)
    return out


# ---- edges --------------------------------------------------------------------------------------------------------
def _edge_cases():
    out = []

    def pair(name, velo2img, good, bad, bad_reason, pixel):
        """Two points, the accepted neighbour and the rejected one, in both orders (so neither hides behind the other)."""
        for order in (0, 1):
            rows = [good, bad] if order == 0 else [bad, good]
            c = _case(f"edge_{name}_{'ab'[order]}", _pts(rows), velo2img)
            r = c["full"]["reason"]
            assert r[order] == spec.ACCEPTED and r[1 - order] == bad_reason, (name, r)
            assert c["n_pixels"] == 1 and c["full"]["winner"][pixel[1], pixel[0]] == order, (name, c["full"]["u"], c["full"]["v"])
            out.append(c)
        return out[-2]["full"]          # of the order (good, bad)

    # h_0 on either side of 2 (uf = h_0 / 1)
    pair("h0_guard", M_PLAIN, (2.0, 3.0, 1.0), (down(2.0), 3.0, 1.0), spec.BELOW_GUARD, (2, 3))
    # uf on either side of 1: 2 / 2 and 2 / nextafter(2)
    pair("uf_low", M_PLAIN, (2.0, 6.0, 2.0), (2.0, 6.0, up(2.0)), spec.OUTSIDE, (1, 3))
    # uf on either side of W
    pair("uf_high", M_PLAIN, (down(W), 3.0, 1.0), (F(W), 3.0, 1.0), spec.OUTSIDE, (W - 1, 3))
    # vf on either side of 1 and of H
    pair("vf_low", M_PLAIN, (6.0, 2.0, 2.0), (6.0, down(2.0), 2.0), spec.OUTSIDE, (3, 1))
    pair("vf_high", M_PLAIN, (3.0, down(H), 1.0), (3.0, F(H), 1.0), spec.OUTSIDE, (3, H - 1))
    # h_2 positive against zero and against negative
    f = pair("h2_zero", M_PLAIN, (4.0, 2.0, 1.0), (4.0, 2.0, 0.0), spec.OUTSIDE, (4, 2))
    assert f["h2"][0] > 0 and f["h2"][1] == 0
    f = pair("h2_negative", M_PLAIN, (4.0, 2.0, 1.0), (4.0, 2.0, -1.0), spec.OUTSIDE, (4, 2))
    assert f["h2"][1] < 0
    # a NaN and an infinite coordinate.  Every h_k has a term in every coordinate, so a NaN anywhere -- and 0 * inf is one --
    # makes h_0 a NaN, which fails the guard; an infinite x under M_PLAIN leaves h_0 infinite and falls at the window
    pair("nan_x", M_PLAIN, (4.0, 2.0, 1.0), (np.nan, 2.0, 1.0), spec.BELOW_GUARD, (4, 2))
    pair("nan_z", M_PLAIN, (4.0, 2.0, 1.0), (4.0, 2.0, np.nan), spec.BELOW_GUARD, (4, 2))
    f = pair("inf_x", M_PLAIN, (4.0, 2.0, 1.0), (np.inf, 2.0, 1.0), spec.OUTSIDE, (4, 2))
    assert np.isnan(f["h2"][1])
    pair("inf_z", M_PLAIN, (4.0, 2.0, 1.0), (4.0, 2.0, np.inf), spec.BELOW_GUARD, (4, 2))
    pair("neg_inf_x", M_PLAIN, (4.0, 2.0, 1.0), (-np.inf, 2.0, 1.0), spec.BELOW_GUARD, (4, 2))
    # the all-zero point passes the guard and the window under M_SHIFT and falls at its range of 0
    pair("zero_point", M_SHIFT, (1.0, 1.0, 0.0), (0.0, 0.0, 0.0), spec.NO_RANGE, (5, 3))
    # uf beyond what an int holds: it has to fall at the float comparison, in front of the cast
    pair("uf_beyond_int", M_PLAIN, (4.0, 2.0, 1.0), (4.0e9, 2.0, 1.0), spec.OUTSIDE, (4, 2))
    pair("uf_huge", M_PLAIN, (4.0, 2.0, 1.0), (4.0, 2.0, 1e-30), spec.OUTSIDE, (4, 2))
    with np.errstate(all="ignore"):
        assert F(4.0e9) / F(1) > F(2 ** 31)
    return out


# ---- known answers ------------------------------------------------------------------------------------------------
def _axis_case():
    """A point on the optical axis lands at (cx, cy) truncated, and there -- x = y = 0 -- the depth is the range to the bit."""
    M = np.array([[50, 0, 30, 0], [0, 40, 22, 0], [0, 0, 1, 0]], F)       # [K | 0] of K_SMALL: the sensor frame is the camera's
    c = _case("axis_point", _pts([(0.0, 0.0, 2.0)]), M)
    assert c["full"]["reason"][0] == spec.ACCEPTED and (c["full"]["u"][0], c["full"]["v"][0]) == (30, 22)
    assert c["range"][22, 30] == F(2) and c["depth"][22, 30].view(np.uint32) == c["range"][22, 30].view(np.uint32)
    assert c["n_pixels"] == 1
    return c


@functools.lru_cache(maxsize=None)
def small_cases():
    """Every case of the 61 x 45 image, in a fixed order."""
    return tuple([_count_case(n) for n in (0, 1, 63, 64, 65, 4097)] + _collision_cases() + _edge_cases() + [_axis_case()])


# ---- conversion ---------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def conversion_case():
    """A range image with every value the conversion treats on its own, the principal-point pixel and the four corners."""
    r = np.random.default_rng(5).uniform(0.5, 80.0, (H, W)).astype(F)
    special = {(1, 1): F(0), (1, 2): F(-1), (1, 3): F(np.nan), (1, 4): F(np.inf), (1, 5): spec.FLT_MAX, (1, 6): F(1e-40),
               (1, 7): F(-np.inf), (1, 8): F(-0.0)}
    for (v, u), val in special.items():
        r[v, u] = val
    r[22, 30] = F(7.25)
    for v, u in ((0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1)):
        r[v, u] = F(10) + F(v) + F(u)
    d = spec.range_to_depth(r, K_SMALL)
    assert all(d[1, u] == 0 and not np.signbit(d[1, u]) for u in (1, 2, 3, 4, 7, 8))
    assert 0 < d[1, 5] < spec.FLT_MAX and np.isfinite(d[1, 5])
    assert 0 < d[1, 6] < F(1e-40) and d[1, 6] < np.finfo(F).tiny                  # a denormal in, a denormal out
    assert d[22, 30].view(np.uint32) == r[22, 30].view(np.uint32)                   # x = y = 0: rim is 1
    for v, u in ((0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1)):
        assert 0 < d[v, u] < r[v, u]
    assert np.all(d[r > 0] <= r[r > 0]) and np.count_nonzero(d) == np.count_nonzero((r > 0) & np.isfinite(r))
    return {"range": r, "K": K_SMALL, "depth": d}


# ---- calibration --------------------------------------------------------------------------------------------------
def golden_calibration():
    with np.load(GOLDEN) as z:
        return {k: z[k].astype(F) for k in ("P_rect", "R_rect", "R_velo", "t_velo")}


def kitti_scene():
    """S-surf sized for a street: a 4 m cube six metres ahead, in a box of ground and surroundings around the sensor."""
    return synth.SurfScene((200, 200, 200), 0.02, np.array([-2.0, -2.0, 4.0]), h=KITTI_H, w=KITTI_W)


def kitti_scan(k=0):
    """The 64-beam scan of kitti_scene from pose k: every ray returns (~119 000 points)."""
    scene = kitti_scene()
    cal = golden_calibration()
    velo2cam = np.eye(4)
    velo2cam[:3, :3], velo2cam[:3, 3] = cal["R_velo"], cal["t_velo"]
    return synth.lidar_scan(scene, scene.pose(k, n=16, max_yaw_deg=5.0), velo2cam, room=(40.0, 25.0, 10.0, 1.73))


@functools.lru_cache(maxsize=None)
def calibration_case():
    cal = golden_calibration()
    velo2img = spec.compose(cal["P_rect"], cal["R_rect"], cal["R_velo"], cal["t_velo"])
    K = np.array([cal["P_rect"][0, 0], 0, cal["P_rect"][0, 2], 0, cal["P_rect"][1, 1], cal["P_rect"][1, 2], 0, 0, 1], F)
    pts = kitti_scan()
    c = _case("kitti_calibration", pts, velo2img, K, KITTI_H, KITTI_W)
    f = c["full"]
    assert 110000 < len(pts) < 125000
    assert c["n_pixels"] > 10000, c["n_pixels"]
    assert not np.any(f["h2"][f["reason"] == spec.ACCEPTED] <= 0)
    assert np.count_nonzero(f["reason"] == spec.BELOW_GUARD) > 10000       # what lies behind the camera
    assert np.count_nonzero(f["reason"] == spec.ACCEPTED) > c["n_pixels"]     # some pixels take more than one point
    return c


# ---- fusing -------------------------------------------------------------------------------------------------------
FUSE_DIMS, FUSE_VS = (48, 40, 36), 0.02
FUSE_H, FUSE_W = 72, 96
FUSE_K = np.array([80.0, 0.0, 47.5, 0.0, 80.0, 35.5, 0.0, 0.0, 1.0], F)
FUSE_ORIGIN = np.array([-0.48, -0.40, 1.0], F)


@functools.lru_cache(maxsize=None)
def fuse_frames():
    """Three scans of S-surf in the 48 x 40 x 36 grid from three poses, with what the restatement makes of them:
    [(cam2world, points, range image, depth image)], and velo2img."""
    scene = synth.SurfScene(FUSE_DIMS, FUSE_VS, FUSE_ORIGIN, K=FUSE_K, h=FUSE_H, w=FUSE_W)
    P = np.zeros((3, 4), F)
    P[:, :3] = FUSE_K.reshape(3, 3)
    velo2img = spec.compose(P, np.eye(3, dtype=F), synth.VELO2CAM[:3, :3].astype(F), synth.VELO2CAM[:3, 3].astype(F))
    frames = []
    for k in (0, 2, 5):
        c2w = scene.pose(k, n=8)
        pts = synth.lidar_scan(scene, c2w, n_azimuth=720, elev_deg=(24.0, -24.0))
        rng_im, n_px = spec.project(pts, velo2img, FUSE_H, FUSE_W)
        assert n_px > 1500, n_px
        frames.append((c2w, pts, rng_im, spec.range_to_depth(rng_im, FUSE_K)))
    return tuple(frames), velo2img
