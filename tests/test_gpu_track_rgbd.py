"""Photometric tracking on the device held to its rule (csrc/tsdf_photo.hip.h) against tests/photo_spec.py over the cases of
tests/photo_cases.py.  The restatement's model is the device's own depth render and the volume's own downloaded colours:

  * tsdf_render_intensity matches the restatement bit for bit, per pixel, at levels 0..2 (odd sizes, invalid pixels);
  * the photometric system of a single pair (a mask on its pixel) equals the double value of the restatement's float32 terms;
  * a system of n pairs is within n * 2^-52 * sum |term| per entry with its count exact, at every size of
    track_cases.REDUCTION; geo_out is tsdf_track_system's output and tsdf_track_rgbd without rgb is tsdf_track, bit for bit;
  * a track's status, iters_run, inliers and photo_pairs are the restatement's, its rmse, photo_rmse and pose entries within
    one float32 ulp (a lost track: the guess's own bits), in cases clear of the restatement's thresholds;
  * facing the textured wall the device ends where the restatement does, within a voxel of the truth; tsdf_track does not;
  * the refusals, and one handle used for one image size after another."""
import ctypes as C

import numpy as np
import pytest

import photo_cases as pc
import photo_spec as ps
import track_cases as tc
import track_spec as ts
from test_gpu_raycast import edge_state
from semantic_slam_amd import capi

pytestmark = pytest.mark.gpu

f32 = np.float32
EYE = np.eye(4, dtype=f32).ravel()


class Rig:
    def __init__(self, torch):
        self.torch = torch
        self.cfg = pc.config()
        self.vols, states = {}, {}
        for kind in ("scene", "wall"):
            v = self.vols[kind] = capi.Volume(self.cfg)
            v.colour_enable()
            for pose, depth, rgb in pc.fuse_frames(kind):
                v.integrate_rgbd(depth, rgb, pose)
        e = self.vols["edge"] = capi.Volume(self.cfg)
        e.upload(*edge_state(pc.DIMS, np.random.default_rng(tc.EDGE_SEED)))
        e.colour_enable()
        e.upload_colour(pc.edge_colours(int(np.prod(pc.DIMS)), np.random.default_rng(52)))
        for k, v in self.vols.items():
            states[k] = v.download() + (v.download_colour(),)
        self.world = pc.PhotoWorld(states, self.render)

    def render(self, volume, ray, pose):
        o = self.vols[volume].raycast(pose, params=ray, normals=True)
        return o["depth"], o["normal"]

    def fresh(self, kind="scene"):
        v = capi.Volume(self.cfg)
        t, w, c = self.world.states[kind]
        v.upload(t, w)
        v.colour_enable()
        v.upload_colour(c)
        return v

    def systems(self, c, vol=None):
        return (vol or self.vols[c.volume]).track_rgbd_system(c.live, c.rgb, c.ref, c.cur, level=c.level, params=c.params(),
                                                              photo=c.photo(), mask=c.mask)

    def track(self, c, vol=None):
        return (vol or self.vols[c.volume]).track_rgbd(c.live, c.rgb, c.ref, params=c.params(), photo=c.photo(), mask=c.mask)

    def dev(self, a):
        return None if a is None else self.torch.from_numpy(np.array(a, order="C")).cuda()

    def geo_system(self, c):
        """tsdf_track_system's 29 sums on the same frame."""
        d, m = self.dev(c.live), self.dev(c.mask)
        A, b, r2, n = self.vols[c.volume].track_system(d.data_ptr(), c.ref, c.cur, level=c.level, params=c.params(),
                                                       mask_ptr=None if m is None else m.data_ptr())
        return np.concatenate([A[np.triu_indices(6)], b, [r2, float(n)]])

    def geo_track(self, c):
        d, m = self.dev(c.live), self.dev(c.mask)
        return self.vols[c.volume].track(d.data_ptr(), c.ref, params=c.params(), mask_ptr=None if m is None else m.data_ptr())

    def close(self):
        for v in self.vols.values():
            v.close()


@pytest.fixture(scope="module")
def rig(cuda):
    r = Rig(cuda)
    yield r
    r.close()


# ------------------------------------------------------------------------------------------------------------------------
# the model intensity image
# ------------------------------------------------------------------------------------------------------------------------
def ray_of(hw, K, thr=0.9):
    c = pc.PhotoCase("ray", np.zeros(hw, f32), None, None, EYE, K=K, hw=hw, thr=thr)
    return c.params().ray


@pytest.mark.parametrize("volume, thr", [("scene", 0.9), ("wall", 0.9), ("edge", 0.9), ("edge", 0.0)])
def test_render_intensity_is_the_restatement_bit_for_bit(rig, volume, thr):
    sc = pc.geometry("scene")
    seen = 0
    for hw in (pc.HW, (33, 66), (5, 7), (1, 1)):
        K = tc.k_for(hw)
        ray = ray_of(hw, K, thr)
        for pose in (sc.pose(9), sc.pose(3)):
            d, _ = rig.render(volume, ray, pose)
            _, w, c = rig.world.states[volume]
            r = {"K": K, "hw": hw, "near": ray.near_m, "far": ray.far_m, "wthr": ray.weight_thresh}
            want = ps.pyramid(ps.model_intensity(d, c, w, pc.DIMS, rig.world.origin, pc.VS, r, pose))
            for level in range(3):
                got = rig.vols[volume].render_intensity(pose, level=level, params=ray)
                assert got.shape == want[level].shape == (hw[0] >> level, hw[1] >> level)
                bad = got.view(np.uint32) != want[level].view(np.uint32)
                assert not bad.any(), f"{volume} {hw} level {level}: {int(bad.sum())} pixels differ, first {np.argwhere(bad)[:3]}"
            if hw == pc.HW:
                inv = float((want[0] < 0).mean())
                seen += 1
                assert inv < 1.0 and (volume != "edge" or 0.02 < inv), (volume, inv)       # valid and invalid pixels both
                assert float((want[0] >= 0).mean()) > 0.02
    assert seen == 2


# ------------------------------------------------------------------------------------------------------------------------
# systems
# ------------------------------------------------------------------------------------------------------------------------
def check_system(rig, c, min_pairs=0):
    """Both systems of one call: the photometric one within the summation bound with its count exact, the geometric one
    tsdf_track_system's own bits; returns (terms, info) of the restatement."""
    info = {}
    terms = pc.spec_terms(rig.world, c, info)
    want, bound = tc.system_bound(terms)
    geo, got = rig.systems(c)
    assert got[28] == len(terms), f"{c}: {got[28]} photometric pairs, spec {len(terms)}"
    assert len(terms) >= min_pairs, (c, len(terms))
    bad = ~(np.abs(got - want) <= bound)
    assert not bad.any(), f"{c}: entries {np.nonzero(bad)[0].tolist()} differ: {got[bad]} vs {want[bad]} (bound {bound[bad]})"
    assert geo.tobytes() == rig.geo_system(c).tobytes(), f"{c}: geo_out is not tsdf_track_system's"
    return terms, info


def check_single_pairs(rig, c, terms, info, picks):
    for idx in picks:
        one = c.but(f"pair {idx}", mask=pc.single_mask(c.hw, c.level, idx))
        _, got = rig.systems(one)
        want = terms[np.searchsorted(info["idx"], idx)].astype(np.float64)
        assert want[28] == 1.0
        assert np.all(got == want), f"{c} sample {idx}: entries {np.nonzero(got != want)[0].tolist()}: {got} vs {want}"
    return len(picks)


def spread(info, n):
    idx = np.asarray(info["idx"])
    return [int(x) for x in idx[np.linspace(0, idx.size - 1, min(n, idx.size)).astype(int)]] if idx.size else []


def test_branch_cases(rig):
    singles = 0
    for name, (c, _) in pc.branch_cases().items():
        if c.mask is not None:                      # (a single-pair mask would replace the case's own)
            check_system(rig, c)
            continue
        terms, info = check_system(rig, c)
        singles += check_single_pairs(rig, c, terms, info, spread(info, 6))
    at, beyond = pc.threshold_cases(rig.world)
    (ta, _), (tb, _) = check_system(rig, at, 100), check_system(rig, beyond, 100)
    assert len(ta) > len(tb)
    print(f"branches: {singles} single-pair systems")
    assert singles >= 60


def test_edge_volume_systems(rig):
    for c in pc.fill_edge_live(rig.world, pc.edge_cases()):
        terms, info = check_system(rig, c, min_pairs=20)
        assert info["rejected"]["invalid_intensity"] > 0
        check_single_pairs(rig, c, terms, info, spread(info, 5))


@pytest.mark.parametrize("hw", tc.REDUCTION, ids=[f"{w}x{h}" for h, w in tc.REDUCTION])
def test_reduction_geometry(rig, hw):
    check_system(rig, pc.reduction_case(hw), min_pairs=50)
    c = pc.reduction_case(hw, close=True)
    terms, info = check_system(rig, c, min_pairs=50)
    picks = tc.nearest_pairs(info["idx"], tc.reduction_targets(hw))
    assert len(picks) >= 4, picks
    check_single_pairs(rig, c, terms, info, picks)
    mask, first = tc.last_workgroup_mask(hw)
    _, li = check_system(rig, c.but("last workgroup", mask=mask), min_pairs=1)
    assert li["idx"].min() >= first


# ------------------------------------------------------------------------------------------------------------------------
# tracks
# ------------------------------------------------------------------------------------------------------------------------
def check_track(rig, c, vol=None):
    hist = []
    want = pc.spec_track(rig.world, c, hist)
    assert tc.preconditions(hist, c.P()) == [], c
    got, st = rig.track(c, vol)
    assert (st["status"], st["iters_run"], st["inliers"], st["photo_pairs"]) == \
        (want["status"], want["iters_run"], want["inliers"], want["photo_pairs"]), f"{c}: {st} vs {want}"
    assert tc.ulps32(st["rmse"], want["rmse32"]) <= 1.0, f"{c}: rmse {st['rmse']!r} vs {want['rmse32']!r}"
    assert tc.ulps32(st["photo_rmse"], want["photo_rmse32"]) <= 1.0, f"{c}: photo_rmse {st['photo_rmse']!r} vs {want['photo_rmse32']!r}"
    if want["lost"]:
        assert got.tobytes() == c.ref.tobytes(), f"{c}: a lost track returns the guess's own bits"
        return got, st, want
    u = tc.ulps32(got.ravel(), want["pose"])
    assert u.max() <= 1.0, f"{c}: pose entries {np.nonzero(u > 1.0)[0].tolist()} off by {u[u > 1.0]} float32 ulps"
    return got, st, want


def test_tracks_follow_the_restatement(rig):
    clear = pc.clear_cases(rig.world, pc.convergence_cases())
    print(f"{len(clear)} convergence candidates are clear of the thresholds: {clear}")
    assert len(clear) >= pc.MIN_CLEAR
    for c in clear:
        _, st, _ = check_track(rig, c)
        assert st["status"] != 2 and st["photo_pairs"] > 1000


def test_state_cases(rig):
    none, zero, few = pc.state_cases()
    _, st, _ = check_track(rig, none)
    assert st["photo_pairs"] == 0 and st["status"] != 2
    for c in (zero, few):
        _, st, _ = check_track(rig, c)
        assert st["status"] == 2


def test_without_rgb_it_is_tsdf_track(rig):
    for c in pc.convergence_cases()[:2] + [pc.convergence_cases()[6]] + pc.state_cases()[1:]:
        want_pose, want = rig.geo_track(c)
        for variant in (c.but("no rgb", rgb=None), c.but("weight 0", weight=0.0)):
            pose, st = rig.track(variant)
            assert pose.tobytes() == want_pose.tobytes(), variant
            assert st["photo_pairs"] == 0 and st["photo_rmse"] == 0.0
            for k, v in want.items():
                assert st[k] == v and type(st[k]) is type(v), (variant, k, st[k], v)


def test_the_wall(rig):
    case, true = pc.wall_case()
    start = pc.in_plane_error(case.ref, true)
    pose, st, want = check_track(rig, case)
    e = pc.in_plane_error(pose, true)
    g_pose, g_st = rig.geo_track(case)
    e_geo = pc.in_plane_error(g_pose, true)
    print(f"wall on the device: guess {start * 1e3:.2f} mm off; combined status {st['status']}, {e * 1e3:.3f} mm "
          f"({st['photo_pairs']} photometric pairs, photo rmse {st['photo_rmse']:.4f}); tsdf_track status {g_st['status']}, "
          f"{e_geo * 1e3:.3f} mm")
    assert st["status"] != 2 and e <= pc.VS
    assert g_st["status"] == 2 or e_geo > 0.5 * start


# ------------------------------------------------------------------------------------------------------------------------
# one handle, one size after another
# ------------------------------------------------------------------------------------------------------------------------
def test_handle_history(rig):
    big, small = (237, 331), (17, 17)
    K = tc.k_for(big)
    true, depth, rgb = pc.scene_frame(K=K, hw=big)
    guess = tc.guess_of(pc.geometry("scene", K, big), true, 80, False)
    track_big = pc.PhotoCase("g 331x237 track", depth, rgb, None, guess, K=K, hw=big, iters=(2, 2, 2))
    sys_big = pc.PhotoCase("g 331x237 system level 2", depth, rgb, None, guess, cur=true, level=2, K=K, hw=big)
    calls = [track_big, pc.reduction_case(small), sys_big, track_big.but("no rgb", rgb=None), track_big]

    def run(vol, c):
        if c.cur is None:
            pose, st = rig.track(c, vol)
            return pose.tobytes() + repr(sorted(st.items())).encode()
        return b"".join(x.tobytes() for x in rig.systems(c, vol))

    with rig.fresh() as used:
        for k, c in enumerate(calls):
            got = run(used, c)
            with rig.fresh() as new:
                want = run(new, c)
            assert got == want, f"call {k} ({c}) on a used handle differs from a fresh one"
        for level in range(3):
            a = used.render_intensity(true, level=level, params=track_big.params().ray)
            b = rig.vols["scene"].render_intensity(true, level=level, params=track_big.params().ray)
            assert a.tobytes() == b.tobytes()


# ------------------------------------------------------------------------------------------------------------------------
# refusals
# ------------------------------------------------------------------------------------------------------------------------
def test_refusals(rig):
    lib = capi.load()
    cfg = capi.make_config((64, 32, 16), 0.01, [0, 0, 0.5], im_height=24, im_width=32)
    hw = (24, 32)
    depth, rgb = np.ones(hw, f32), np.zeros(hw + (3,), np.uint8)
    res, g29, p29, img = capi.TrackRgbdResult(), np.zeros(29), np.zeros(29), np.zeros(hw, f32)
    good, photo = capi.track_params_default(cfg), capi.photo_params_default(cfg)

    def refused(h, what, p=good, pp=photo, d=depth, c=rgb, out=True, level=0, which="track", pose=EYE):
        ptr = lambda a: None if a is None else a.ctypes.data
        if which == "system":
            rc = lib.tsdf_track_rgbd_system(h, C.byref(p), None if pp is None else C.byref(pp), ptr(d), ptr(c), None, ptr(pose),
                                            ptr(pose), level, g29.ctypes.data if out else None, p29.ctypes.data)
        elif which == "track":
            rc = lib.tsdf_track_rgbd(h, C.byref(p), None if pp is None else C.byref(pp), ptr(d), ptr(c), None, ptr(pose),
                                     C.byref(res) if out else None)
        else:
            rc = lib.tsdf_render_intensity(h, C.byref(p.ray), ptr(pose), level, img.ctypes.data if out else None)
        msg = lib.tsdf_last_error().decode()
        assert rc == -1 and what in msg, (which, rc, msg)

    with capi.Volume(cfg) as plain:
        refused(plain._h, "tsdf_colour_enable")
        refused(plain._h, "tsdf_colour_enable", which="system")
        refused(plain._h, "tsdf_colour_enable", which="render")
        plain.track_rgbd(depth, None, EYE, params=good)                 # depth only needs no colour
    with capi.Volume(cfg) as vol:
        vol.colour_enable()
        for which in ("track", "system"):
            refused(vol._h, "NULL depth", d=None, which=which)
            refused(vol._h, "NULL result", out=False, which=which)
            refused(vol._h, "NULL photometric", pp=None, which=which)
            refused(vol._h, "NULL argument", pose=None, which=which)
            for field, value in (("photo_weight", -0.5), ("photo_weight", float("nan")), ("photo_weight", float("inf")),
                                 ("intensity_thresh", 0.0), ("intensity_thresh", -1.0), ("intensity_thresh", float("nan")),
                                 ("intensity_thresh", float("inf"))):
                pp = capi.photo_params_default(cfg)
                setattr(pp, field, value)
                refused(vol._h, field, pp=pp, which=which)
            for field, value, what in (("n_levels", 0, "n_levels"), ("n_levels", 4, "n_levels"),
                                       ("cos_normal_thresh", 1.5, "cos_normal_thresh"), ("eps_rot", 0.0, "eps_rot"),
                                       ("min_inliers", -1, "min_inliers")):
                p = capi.track_params_default(cfg)
                setattr(p, field, value)
                refused(vol._h, what, p=p, which=which)
            p = capi.track_params_default(cfg)
            p.dist_thresh[1] = float("nan")
            refused(vol._h, "dist_thresh[1]", p=p, which=which)
            p = capi.track_params_default(cfg)
            p.iters[2] = -1
            refused(vol._h, "iters[2]", p=p, which=which)
            p = capi.track_params_default(cfg)
            p.ray.near_m = -1.0
            refused(vol._h, "near", p=p, which=which)
        refused(vol._h, "NULL argument", c=None, which="system")
        refused(vol._h, "level 3 is outside", level=3, which="system")
        refused(vol._h, "level -1 is outside", level=-1, which="system")
        refused(vol._h, "level 3 is outside", level=3, which="render")
        refused(vol._h, "level -1 is outside", level=-1, which="render")
        refused(vol._h, "NULL argument", out=False, which="render")
        refused(vol._h, "NULL argument", pose=None, which="render")
        vol.track_rgbd(depth, rgb, EYE, params=good)                     # and good calls still work
        vol.render_intensity(EYE, level=2, params=good.ray)
    with capi.Volume(capi.make_config((64, 32, 16), 0.01, [0, 0, 0.5], z_begin=4, z_end=12, im_height=24, im_width=32)) as slab:
        slab.colour_enable()
        for which in ("track", "system", "render"):
            refused(slab._h, "z-slab", which=which)
    g = C.c_void_p()
    devs = (C.c_int32 * 1)(0)
    assert lib.tsdf_group_create(C.byref(cfg), devs, 1, C.byref(g)) == 0
    try:
        h = C.c_void_p()
        assert lib.tsdf_group_volume(g, 0, C.byref(h)) == 0
        refused(h, "tsdf_group", c=None)
        refused(h, "tsdf_group", which="render")
    finally:
        lib.tsdf_group_destroy(g)
