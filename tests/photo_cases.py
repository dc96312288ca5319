"""The coloured scenes and named cases of tests/test_photo_spec.py (CPU) and tests/test_gpu_track_rgbd.py (device), test
infrastructure on top of tests/track_cases.py: the same grid (DIMS, VS), image (HW, K_SMALL) and reduction sizes, with colour.

Two scenes, each fused with colour from FUSE_POSES 320 x 240 frames: "scene", track_cases' TrackScene (two spheres in front of
a wall), and "wall", the same scene without its spheres: a fronto-parallel plane.  Both carry texture(): a sum of three sines
of the surface point's base-frame x and y whose shortest wavelength (0.10 m) is 16.7 voxel edges, above the 8 the wall test
asks for.  A PhotoWorld holds the volumes' states (tsdf, weight, colour) and a depth / normal renderer -- raycast_spec on the
CPU, the device's own render on the GPU -- and derives the model intensity pyramid with photo_spec from the state.  Every
perturbation, mask and threshold below is computed on the CPU; nothing here reads a device result but the render."""
import math

import numpy as np

import photo_spec as ps
import track_cases as tc
import track_spec as ts
from semantic_slam_amd import capi, synth

f32 = np.float32
DIMS, VS, Z0, HW, K_SMALL = tc.DIMS, tc.VS, tc.Z0, tc.HW, tc.K_SMALL
FUSE_HW = (240, 320)
FUSE_K = (synth.TUM_K.astype(np.float64) * np.array([.5, 1, .5, 1, .5, .5, 1, 1, 1])).astype(f32)
FUSE_POSES = (0, 8, 16, 24, 40, 56)
LAMBDAS = (0.10, 0.13, 0.16)        # metres; the third runs along x + y, so its wavelength is 0.16 / sqrt(2) = 0.113 m
assert min(LAMBDAS[0], LAMBDAS[1], LAMBDAS[2] / math.sqrt(2.0)) >= 8 * VS


def origin_of():
    return synth.surf_volume(max(DIMS), VS, Z0)


def geometry(kind, K=K_SMALL, hw=HW):
    sc = synth.TrackScene(DIMS, VS, origin_of(), K=K, h=hw[0], w=hw[1])
    if kind == "wall":
        sc.spheres = []
    return sc


def texture(P):
    """uint8 RGB [..., 3] of base-frame points P [..., 3]."""
    x, y = P[..., 0], P[..., 1]
    w = [2.0 * math.pi / l for l in LAMBDAS]
    r = 128.0 + 50.0 * np.sin(w[0] * x) + 45.0 * np.sin(w[1] * y + 0.7) + 25.0 * np.sin(w[2] * (x + y))
    g = 128.0 + 50.0 * np.sin(w[0] * x + 1.1) + 45.0 * np.sin(w[1] * y) + 25.0 * np.sin(w[2] * (x + y) + 2.0)
    b = 100.0 + 40.0 * np.sin(w[1] * x + 0.4)
    return np.clip(np.round(np.stack([r, g, b], axis=-1)), 0, 255).astype(np.uint8)


def frame(sc, pose):
    """(depth [H, W] float32 quantised as the sensor's, rgb [H, W, 3] uint8; black where nothing is hit)."""
    T, d, z, _ = sc._hit(pose)
    hit = np.isfinite(z)
    P = T[:3, 3] + np.where(hit, z, 0.0)[..., None] * d
    rgb = np.where(hit[..., None], texture(P), 0).astype(np.uint8)
    return sc.depth(pose, quantize=True), np.ascontiguousarray(rgb)


def fuse_frames(kind):
    sc = geometry(kind, FUSE_K, FUSE_HW)
    return [(sc.pose(k),) + frame(sc, sc.pose(k)) for k in FUSE_POSES]


def config():
    return capi.make_config(DIMS, VS, origin_of(), K=FUSE_K, im_height=FUSE_HW[0], im_width=FUSE_HW[1])


def cpu_fuse(kind):
    """(tsdf, weight, colour) flat x-fastest: projective TSDF fusion with the running colour mean, in NumPy.  It stands in for
    the device's Integrate and colour passes on the CPU only; it is a volume to track against, not a parity reference."""
    dx, dy, dz = DIMS
    o = origin_of().astype(np.float64)
    trunc = float(f32(VS) * f32(5))
    z, y, x = np.meshgrid(np.arange(dz), np.arange(dy), np.arange(dx), indexing="ij")
    P = np.stack([o[0] + x.ravel() * VS, o[1] + y.ravel() * VS, o[2] + z.ravel() * VS], axis=1)
    n = P.shape[0]
    t, w, c = np.ones(n), np.zeros(n), np.zeros((n, 3))
    K = FUSE_K.astype(np.float64)
    for pose, depth, rgb in fuse_frames(kind):
        T = np.asarray(pose, np.float64).reshape(4, 4)
        pc = (P - T[:3, 3]) @ T[:3, :3]
        with np.errstate(divide="ignore", invalid="ignore"):
            pu = np.round(K[0] * pc[:, 0] / pc[:, 2] + K[2])
            pv = np.round(K[4] * pc[:, 1] / pc[:, 2] + K[5])
        ok = (pc[:, 2] > 0) & (pu >= 0) & (pu < FUSE_HW[1]) & (pv >= 0) & (pv < FUSE_HW[0])
        iu, iv = np.where(ok, pu, 0).astype(int), np.where(ok, pv, 0).astype(int)
        d = depth[iv, iu].astype(np.float64)
        diff = d - pc[:, 2]
        upd = ok & (d > 0) & (d <= 6.0) & (diff > -trunc)
        wn = w + 1.0
        t = np.where(upd, (t * w + np.minimum(1.0, diff / trunc)) / wn, t)
        c = np.where(upd[:, None], (c * w[:, None] + rgb[iv, iu]) / wn[:, None], c)
        w = np.where(upd, wn, w)
    ci = np.clip(np.round(c), 0, 255).astype(np.uint32)
    return t.astype(f32), w.astype(f32), (ci[:, 2] << 16) | (ci[:, 1] << 8) | ci[:, 0]


def edge_colours(n, rng):
    """Random colours for the value-edge volume, extremes included."""
    c = rng.integers(0, 1 << 24, n, dtype=np.uint32)
    c[rng.choice(n, n // 20, replace=False)] = 0x00FFFFFF
    c[rng.choice(n, n // 20, replace=False)] = 0
    return c


class PhotoWorld:
    """states: {name: (tsdf, weight, colour)}; render(name, ray, pose) -> (depth [H, W], normal [H, W, 3])."""

    def __init__(self, states, render):
        self.states, self.origin = states, origin_of()
        self.base = tc.World(DIMS, VS, self.origin, render)

    def model(self, case):
        ray = case.params().ray
        d, n = self.base.render(case.volume, ray, case.ref)
        _, w, c = self.states[case.volume]
        r = {"K": case.K, "hw": case.hw, "near": ray.near_m, "far": ray.far_m, "wthr": ray.weight_thresh}
        I0 = ps.model_intensity(d, c, w, DIMS, self.origin, VS, r, case.ref)
        return d, n, ps.pyramid(I0)


class PhotoCase(tc.Case):
    def __init__(self, name, live, rgb, mask, ref, weight=ps.DEFAULT_WEIGHT, ithr=ps.DEFAULT_ITHR, **kw):
        super().__init__(name, live, mask, ref, **kw)
        self.rgb = None if rgb is None else np.ascontiguousarray(rgb, np.uint8)
        self.weight, self.ithr = weight, ithr

    def photo(self):
        return capi.PhotoParams(self.weight, self.ithr)

    def PP(self):
        return ps.photo_params(self.weight, self.ithr)

    def live_tuple(self):
        return self.live, self.mask, None if self.rgb is None else ps.live_pyramid(self.rgb)

    def but(self, name, **kw):
        c = PhotoCase.__new__(PhotoCase)
        c.__dict__.update(self.__dict__)
        c.par = dict(self.par)
        for k, v in kw.items():
            if k in c.par:
                c.par[k] = v
            else:
                setattr(c, k, v)
        c.name = f"{self.name} {name}"
        return c


def spec_terms(world, case, info=None):
    M = ts.relative(case.ref, case.cur)
    terms, _ = ps.pair_terms(case.live_tuple(), world.model(case), case.level, M[:, :3].astype(f32), M[:, 3].astype(f32),
                             case.P(), case.PP(), info)
    return terms


def spec_track(world, case, history=None):
    r = ps.track(case.live_tuple(), world.model(case), case.P(), case.PP(), history=history)
    r["pose"] = case.ref.copy() if r["lost"] else ts.result_pose(np.eye(4, dtype=f32), case.ref, r["M"])
    r["rmse32"], r["photo_rmse32"] = f32(r["rmse"]), f32(r["photo_rmse"])
    return r


def single_mask(hw, level, idx):
    """A mask that is >= 128 on exactly the pixel of flat sample idx of the level (a photometric pair reads one depth)."""
    u, v, _ = ts.sample_grid(hw, level)
    m = np.zeros(hw, np.uint8)
    m[v[idx], u[idx]] = 255
    return m


# ------------------------------------------------------------------------------------------------------------------------
# system cases: one per branch of the rule
# ------------------------------------------------------------------------------------------------------------------------
def scene_frame(kind="scene", k=9, K=K_SMALL, hw=HW):
    sc = geometry(kind, K, hw)
    true = sc.pose(k)
    return (true,) + frame(sc, true)


def branch_cases():
    """{name: (case, gate that must reject at least one sample, or None)} on the scene volume."""
    true, depth, rgb = scene_frame()
    ref = ts.perturb(true, np.random.default_rng(40), 1.0, 0.01)
    out = {}
    for level in range(3):
        out[f"plain level {level}"] = (PhotoCase(f"plain level {level}", depth, rgb, None, ref, cur=true, level=level), None)
    base = out["plain level 0"][0]
    # the render has no model where rays leave the grid or cross a silhouette: footprints that straddle such pixels
    out["invalid model intensity"] = (base.but("invalid model"), "invalid_intensity")
    # p = M V with M = C_ref^-1 C_cur: a camera moved along +x of its own frame sends the points off the RIGHT of the model
    for side, t in (("right", (0.2, 0, 0)), ("left", (-0.2, 0, 0)), ("bottom", (0, 0.12, 0)), ("top", (0, -0.12, 0))):
        out[f"footprint off the {side}"] = (base.but(f"off the {side}", cur=tc.moved(true, t_cam=t), dist=(10.0,) * 3),
                                            "footprint")
    out["occluded in front"] = (base.but("in front", cur=tc.moved(ref, t_cam=(0, 0, 0.03)), dist=(0.01,) * 3), "occluded")
    out["occluded behind"] = (base.but("behind", cur=tc.moved(ref, t_cam=(0, 0, -0.03)), dist=(0.01,) * 3), "occluded")
    bad = depth.copy()
    bad[10:30, 20:60] = np.nan
    bad[50:60, 100:120] = np.inf
    out["NaN depth"] = (base.but("NaN depth", live=bad), "depth_or_mask")
    mask = np.full(HW, 255, np.uint8)
    mask[::3, ::2] = 127
    mask[40:70, 30:90] = 0
    out["masked pixel"] = (base.but("masked", mask=mask), "depth_or_mask")
    tiny = (5, 5)
    Kt = tc.k_for(tiny)
    t_true, t_depth, t_rgb = scene_frame(K=Kt, hw=tiny)
    out["level too small"] = (PhotoCase("5x5 level 2", t_depth, t_rgb, None, t_true, cur=t_true, level=2, K=Kt, hw=tiny,
                                        dist=(10.0,) * 3), "footprint")
    return out


def threshold_cases(world):
    """(at, beyond): intensity_thresh equal to one sample's |r| (that sample pairs) and one float32 below it (it does not)."""
    base = branch_cases()["plain level 0"][0].but("thr", ithr=1.0)
    info = {}
    spec_terms(world, base, info)
    r = np.sort(np.abs(info["r"]))
    thr = float(r[int(0.9 * r.size)])
    assert thr > 0.0
    return base.but("at", ithr=thr), base.but("beyond", ithr=float(np.nextafter(f32(thr), f32(0))))


def edge_cases():
    """The value-edge volume with random colours: invalid and valid corners mixed, at two weight thresholds."""
    sc = geometry("scene")
    ref = sc.pose(3)
    cur = ts.perturb(ref, np.random.default_rng(50), 1.0, 0.01)
    rng = np.random.default_rng(51)
    rgb = rng.integers(0, 256, HW + (3,), dtype=np.uint8)
    out = []
    for thr in (0.9, 0.0):
        for level in (0, 2):
            out.append(PhotoCase(f"edge thr {thr} level {level}", np.zeros(HW, f32), rgb, None, ref, cur=cur, level=level,
                                 volume="edge", thr=thr, ithr=1.0))
    return out


def fill_edge_live(world, cases):
    for c in cases:
        c.live = np.array(world.base.render("edge", c.params().ray, c.cur)[0])
    return cases


def reduction_case(hw, close=False):
    """track_cases.reduction_case with colour: level 0 of hw, straight on with the longer lens."""
    K = tc.k_for(hw, tc.K_LONG)
    true, depth, rgb = scene_frame(k=0, K=K, hw=hw)
    ref = ts.perturb(true, np.random.default_rng(70), 0.05 if close else 1.0, 0.0005 if close else 0.01)
    return PhotoCase(f"e {hw[1]}x{hw[0]}{' close' if close else ''}", depth, rgb, None, ref, cur=true, level=0, K=K, hw=hw)


# ------------------------------------------------------------------------------------------------------------------------
# tracked cases
# ------------------------------------------------------------------------------------------------------------------------
MIN_INLIERS = 100


def convergence_cases():
    """Perturbed guesses on the scene, 1 deg / 1 cm: candidates, of which clear_cases keeps those the restatement decides
    away from its own thresholds."""
    true, depth, rgb = scene_frame()
    sc = geometry("scene")
    out = []
    for seed in (61, 62, 63, 64, 65, 66):
        out.append(PhotoCase(f"track seed {seed}", depth, rgb, None, tc.guess_of(sc, true, seed, False), min_inliers=MIN_INLIERS))
    mask = np.zeros(HW, np.uint8)
    mask[HW[0] // 8: HW[0] - HW[0] // 8, HW[1] // 9: HW[1] - HW[1] // 8] = 255
    out.append(PhotoCase("track seed 61 mask", depth, rgb, mask, tc.guess_of(sc, true, 61, False), min_inliers=MIN_INLIERS))
    out.append(out[0].but("levels 2 iters (3, 2)", n_levels=2, iters=(3, 2, 0)))
    return out


MIN_CLEAR = 5         # of the 8 candidates


def clear_cases(world, cases):
    """The cases whose restatement track breaches none of track_cases.preconditions (a step within 10 % of eps, a pivot within
    a factor 2 of lost): equality of the state machine means something only there."""
    out = []
    for c in cases:
        h = []
        spec_track(world, c, h)
        if not tc.preconditions(h, c.P()):
            out.append(c)
    return out


def state_cases():
    """Tracks whose outcome is decided by a count, not by a threshold on a float."""
    true, depth, rgb = scene_frame()
    g = tc.guess_of(geometry("scene"), true, 61, False)
    return [PhotoCase("no photometric pairs", depth, rgb, None, g, ithr=1e-9, min_inliers=MIN_INLIERS, iters=(2, 2, 2)),
            PhotoCase("lost: all-zero depth", np.zeros(HW, f32), rgb, None, g, min_inliers=MIN_INLIERS),
            PhotoCase("lost: min_inliers", depth, rgb, None, g, min_inliers=10 ** 6)]


WALL_SHIFT = 0.015     # metres along the wall's x: 3.7 level-0 pixel footprints (z / fx = 1.203 / 300 = 4.0 mm), 2.5 voxel edges


def wall_case():
    """The fronto-parallel wall seen straight on; the guess is the truth shifted by WALL_SHIFT in the plane."""
    sc = geometry("wall")
    true = sc.pose(0)
    depth, rgb = frame(sc, true)
    z = float(depth[HW[0] // 2, HW[1] // 2])
    assert WALL_SHIFT >= 3.0 * z / float(K_SMALL[0])
    guess = tc.moved(true, t_cam=(WALL_SHIFT, 0.0, 0.0))
    return PhotoCase("wall", depth, rgb, None, guess, volume="wall", min_inliers=MIN_INLIERS), true


def in_plane_error(pose, true):
    """The distance between two poses' translations within the wall's plane (base x, y), metres."""
    a, b = np.asarray(pose, np.float64).reshape(4, 4), np.asarray(true, np.float64).reshape(4, 4)
    return float(np.hypot(a[0, 3] - b[0, 3], a[1, 3] - b[1, 3]))
