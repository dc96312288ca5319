"""The cases of tests/test_scan_track_spec.py (CPU) and tests/test_gpu_scan_track.py (test infrastructure).  Everything here is
computed once per case and handed out read-only.

The corner world.  A 48^3 grid at 40 mm (truncation 200 mm: the smallest grid that holds an inside corner with its band on
three sides), base frame rotated and shifted against the world.  The scene is the inside corner of three planes, x = 1.5,
y = 1.5 (walls) and z = 0.42 (the floor), in base coordinates; it is fused from six synthetic depth frames through the CPU
oracle, so all six degrees of freedom are constrained.  A synthetic scan is 24 rings of 360 points, ring-major (ring 0 lowest,
azimuth ascending inside a ring) as a spinning scanner delivers them, cast from a scanner inside the corner onto the planes; a
ray that meets none of them returns nothing.  corner_world(BIG) is the same scene 6.25 times as large (250 mm voxels, ranges of
3 ... 10 m), where tsdf_scan_track_params_default's ranges and min_pairs fit as they are.

The exact world.  The same grid size at voxel size 2^-4 with origin (-1, -1, -1), identity poses, every voxel observed
(weight 2) with a smooth field, |t| < 0.9: positions and grid coordinates of hand-placed points are exact, so a comparison can
be put exactly ON its threshold.  A few cells are prepared for the named cases (SPECIAL)."""
import functools
import math

import numpy as np

import fuse_cases as fc
import fuse_spec as fs
import scan_track_spec as sts
import track_spec as ts
from semantic_slam_amd import capi

f32 = np.float32
DIMS = (48, 48, 48)
LEVELS = (0, 1, 2)
MAX_BLOCKS = 256            # csrc/tsdf_track.hip.h: kTrackMaxBlocks

# ------------------------------------------------------------------------------------------------------------------------
# the corner world
# ------------------------------------------------------------------------------------------------------------------------
VS = 0.04
PLANES = (1.5, 1.5, 0.42)                  # x = , y = (hit from below), z = (the floor, hit from above), base coordinates
N_RINGS, N_AZ = 24, 360
ELEV = (-40.0, 30.0)                       # degrees, ring 0 .. ring N_RINGS - 1
SCANNER_AT = (0.62, 0.55, 1.02)


def look_at(eye, target, up=(0.0, 0.0, 1.0)):
    """cam2base [4, 4] float64 of a camera at `eye` looking at `target` (z forward, x right, y down)."""
    eye, target = np.asarray(eye, np.float64), np.asarray(target, np.float64)
    z = (target - eye) / np.linalg.norm(target - eye)
    x = np.cross(z, np.asarray(up, np.float64))
    x /= np.linalg.norm(x)
    y = np.cross(z, x)
    T = np.eye(4)
    T[:3, 0], T[:3, 1], T[:3, 2], T[:3, 3] = x, y, z, eye
    return T


def plane_ranges(o, d, scale=1.0):
    """The distance along the rays o + s d (d [n, 3], base coordinates) to the nearest of the three planes met from inside the
    corner; inf where none is met."""
    o = np.asarray(o, np.float64)
    s = np.full(len(d), np.inf)
    with np.errstate(divide="ignore", invalid="ignore"):
        for a, (P, sign) in enumerate(zip(PLANES, (1.0, 1.0, -1.0))):
            hit = d[:, a] * sign > 1e-9
            s = np.where(hit, np.minimum(s, (P * scale - o[a]) / np.where(hit, d[:, a], 1.0)), s)
    return s


def corner_depth(cam2base, scale=1.0):
    """The z-depth image (fuse_cases.IM_HW, K_SMALL) of the corner from cam2base; 0 where no plane is met."""
    H, W = fc.IM_HW
    K = fc.K_SMALL
    v, u = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    dc = np.stack([(u.ravel() - K[2]) / K[0], (v.ravel() - K[5]) / K[4], np.ones(H * W)], -1)
    d = dc @ cam2base[:3, :3].T
    s = plane_ranges(cam2base[:3, 3], d, scale)
    return np.where(np.isfinite(s), s, 0.0).astype(f32).reshape(H, W)


VIEWS = [((0.30, 0.45, 1.20), (1.5, 1.10, 0.80)), ((0.50, 0.25, 1.10), (1.05, 1.5, 0.85)), ((0.40, 0.40, 1.55), (1.10, 1.10, 0.42)),
         ((0.25, 0.30, 0.95), (1.5, 1.5, 0.60)), ((0.70, 0.30, 1.40), (1.30, 1.5, 0.42)), ((0.30, 0.75, 1.35), (1.5, 1.25, 0.42))]


BIG = 6.25                                 # the corner at the size of a street scene: 250 mm voxels, ranges of 3 ... 10 m


def corner_config(scale=1.0):
    R = ts.rodrigues(np.array([0.1, -0.2, 0.3]))
    b2w = np.eye(4)
    b2w[:3, :3], b2w[:3, 3] = R, (2.0, -1.0, 0.5)
    return capi.make_config(DIMS, VS * scale, np.zeros(3, f32), K=fc.K_SMALL, base2world=b2w.astype(f32).ravel(),
                            im_height=fc.IM_HW[0], im_width=fc.IM_HW[1], max_depth=6.0 * scale)


def corner_frames(scale=1.0):
    """[(depth [H, W] float32, cam2base [4, 4] float64)] of VIEWS."""
    views = [look_at(np.asarray(e) * scale, np.asarray(t) * scale) for e, t in VIEWS]
    return [(corner_depth(c2b, scale), c2b) for c2b in views]


@functools.lru_cache(maxsize=None)
def corner_world(scale=1.0):
    """(cfg, (tsdf, weight), grid): the corner fused through the CPU oracle, read-only."""
    from oracle.oracle import Oracle
    cfg = corner_config(scale)
    grid = fs.grid_of(cfg)
    orc = Oracle()
    t, w = orc.init_grid(DIMS)
    for depth, c2b in corner_frames(scale):
        orc.integrate(fc.K_SMALL, c2b.astype(f32).ravel(), depth, DIMS, grid[1], float(grid[2]), float(grid[3]), t, w,
                      max_depth=float(cfg.max_depth))
    t.setflags(write=False)
    w.setflags(write=False)
    return cfg, (t, w), grid


def ring_directions(n_rings=N_RINGS, n_az=N_AZ, elev=ELEV):
    """Unit directions [n_rings * n_az, 3] in the scanner's frame (x forward, y left, z up), ring-major."""
    el = np.radians(np.linspace(elev[0], elev[1], n_rings))[:, None]
    az = (np.arange(n_az) * (2.0 * math.pi / n_az) - math.pi)[None, :]
    d = np.stack([np.cos(el) * np.cos(az), np.cos(el) * np.sin(az), np.sin(el) * np.ones_like(az)], -1)
    return d.reshape(-1, 3)


@functools.lru_cache(maxsize=None)
def corner_scan(scale=1.0):
    """(points [n, 4] float32, the true velo2world float32 [16]): the scan from SCANNER_AT, the scanner turned a little
    against the base frame."""
    grid = fs.grid_of(corner_config(scale))
    v2b = np.eye(4)
    v2b[:3, :3], v2b[:3, 3] = ts.rodrigues(np.array([0.02, -0.03, 0.4])), np.asarray(SCANNER_AT) * scale
    d = ring_directions()
    s = plane_ranges(v2b[:3, 3], d @ v2b[:3, :3].T, scale)
    ok = np.isfinite(s)
    pts = np.zeros((int(ok.sum()), 4), f32)
    pts[:, :3] = (d[ok] * s[ok, None]).astype(f32)
    pts[:, 3] = 0.5
    pts.setflags(write=False)
    truth = (np.asarray(grid[4], np.float64).reshape(4, 4) @ v2b).astype(f32).ravel()
    return pts, truth


def corner_params(**kw):
    """The defaults with ranges that fit a 2 m room and min_pairs 100.  eps 3e-5, not the default 1e-5: on this scene the second
    iteration of level 1 takes a step of |tau| = 1.01e-5 from every guess tried, within 1 % of the default eps_trans, and a
    run whose state machine hangs on the last bits of a sum is no parity case (preconditions)."""
    cfg, _, _ = corner_world()
    kw.setdefault("eps_rot", 3e-5)
    kw.setdefault("eps_trans", 3e-5)
    kw.setdefault("min_range_m", 0.2)
    kw.setdefault("max_range_m", 10.0)
    kw.setdefault("min_pairs", 100)
    return sts.params(cfg.trunc_margin, **kw)


def ground_params():
    """tsdf_scan_mark_ground's parameters for the corner scan (a scan_ground_spec.Params): its rings and columns, every beam at
    its ring's centre."""
    import scan_ground_spec as sg
    res = (ELEV[1] - ELEV[0]) / (N_RINGS - 1)
    return sg.params(n_rings=N_RINGS, n_columns=N_AZ, ang_res_y=res, ang_bottom=-ELEV[0] + res / 2, ground_rings=N_RINGS - 1)


def moved(velo2world, deg, metres, seed):
    """velo2world with a seeded rigid motion of the scanner's frame in front of it: a rotation of `deg` about a random axis
    through the scanner and a shift of `metres` in a random direction (float64, rounded to float32 [16])."""
    rng = np.random.default_rng(seed)
    ax, d = rng.normal(size=3), rng.normal(size=3)
    T = np.eye(4)
    T[:3, :3] = ts.rodrigues(ax / np.linalg.norm(ax) * math.radians(deg))
    T[:3, 3] = d / np.linalg.norm(d) * metres
    return (np.asarray(velo2world, np.float64).reshape(4, 4) @ T).astype(f32).ravel()


def shifted(velo2world, base_shift):
    """velo2world moved by base_shift (base coordinates) in the volume's frame."""
    b2w = np.asarray(corner_config().base2world, np.float64).reshape(4, 4)
    T = np.eye(4)
    T[:3, 3] = base_shift
    return (b2w @ T @ np.linalg.inv(b2w) @ np.asarray(velo2world, np.float64).reshape(4, 4)).astype(f32).ravel()


# (name, rotation in degrees, translation in metres, seed): inside the basin
INSIDE = [("a translation of two voxels", 0.0, 0.08, 11), ("a rotation of 1.2 degrees", 1.2, 0.0, 12),
          ("1 degree and 60 mm", 1.0, 0.06, 13)]


class RunCase:
    """One tsdf_scan_track call and the restatement's run."""

    def __init__(self, name, vol, grid, cfg, points, flags, P, guess):
        self.name, self.vol, self.grid, self.cfg, self.points, self.flags, self.P = name, vol, grid, cfg, points, flags, P
        self.guess = np.asarray(guess, f32).ravel()
        self._want = None

    def want(self):
        if self._want is None:
            hist = []
            r = sts.track(self.vol, self.grid, self.points, self.flags, self.P, self.guess, hist)
            r["history"], r["rmse32"] = hist, f32(r["rmse"])
            self._want = r
        return self._want

    def __repr__(self):
        return self.name


@functools.lru_cache(maxsize=None)
def convergence_cases():
    cfg, vol, grid = corner_world()
    pts, truth = corner_scan()
    return [RunCase(name, vol, grid, cfg, pts, None, corner_params(), moved(truth, deg, metres, seed))
            for name, deg, metres, seed in INSIDE]


@functools.lru_cache(maxsize=None)
def lost_cases():
    """Outside the basin: every plane displaced by more than the truncation distance; the scan over the part of the grid no
    frame has observed; the scan outside the grid; no points at all."""
    cfg, vol, grid = corner_world()
    pts, truth = corner_scan()
    P = corner_params()
    return [RunCase("every plane off by 0.35 m", vol, grid, cfg, pts, None, P, shifted(truth, (0.35, 0.35, -0.35))),
            RunCase("over the unobserved part of the grid", vol, grid, cfg, pts, None, P, shifted(truth, (-1.2, -1.2, 0.9))),
            RunCase("outside the grid", vol, grid, cfg, pts, None, P, shifted(truth, (40.0, 0.0, 0.0))),
            RunCase("no points", vol, grid, cfg, np.zeros((0, 4), f32), None, P, truth)]


def preconditions(history, P):
    """track_cases.preconditions (a step within 10 % of an eps, a pivot within a factor 2 of the lost threshold), and: a
    computed comparison within one float32 spacing of its threshold (sts.pair_terms' "near") is a breach."""
    import track_cases as tc
    bad = tc.preconditions(history, {"eps_rot": P["eps_rot"], "eps_trans": P["eps_trans"]})
    for k, h in enumerate(history):
        if any(h["near"].values()):
            bad.append((k, "near", h["near"]))
    return bad


# ------------------------------------------------------------------------------------------------------------------------
# the exact world and the named cases
# ------------------------------------------------------------------------------------------------------------------------
EXACT_VS = 2.0 ** -4
EXACT_ORIGIN = (-1.0, -1.0, -1.0)
MIN_RANGE, MAX_RANGE = 0.5, 1.5            # squares 0.25 and 2.25: exact
HALF = f32(0.5)
# voxel indices of the prepared cells (their lowest corner)
SPECIAL = {"weight": (30, 20, 20), "free": (30, 24, 20), "flat": (30, 28, 20), "resid_on": (26, 20, 24), "resid_over": (26, 24, 24)}


def at(i, j, k):
    """The position of grid coordinates (i, j, k) in the exact world (exact in float32 for multiples of 2^-19)."""
    return [EXACT_ORIGIN[0] + i * EXACT_VS, EXACT_ORIGIN[1] + j * EXACT_VS, EXACT_ORIGIN[2] + k * EXACT_VS]


@functools.lru_cache(maxsize=None)
def exact_world():
    """(cfg, (tsdf, weight), grid), read-only."""
    cfg = fc.config(DIMS, EXACT_VS, np.asarray(EXACT_ORIGIN, f32))
    z, y, x = np.meshgrid(*[np.arange(d, dtype=np.float64) for d in DIMS[::-1]], indexing="ij")
    t = 0.012 * (x - 24) + 0.008 * (y - 24) - 0.010 * (z - 24) + 0.05 * np.sin(0.3 * x + 0.2 * y + 0.25 * z)
    t = t.astype(f32)
    assert np.abs(t).max() < 0.9
    w = np.full(t.shape, 2.0, f32)

    def cell(name):
        i, j, k = SPECIAL[name]
        return (slice(k, k + 2), slice(j, j + 2), slice(i, i + 2))

    w[cell("weight")][1, 1, 1] = f32(0.9)                  # one corner exactly AT weight_thresh
    t[cell("free")] = 1.0                                  # eight free-space corners: F = 1 exactly
    t[cell("flat")] = 0.25                                 # a flat field: F = 0.25, zero gradient
    i, j, k = SPECIAL["resid_on"]
    t[k, j, i] = HALF                                      # a point ON this voxel has F = 0.5 exactly, r = 0.5 * trunc
    i, j, k = SPECIAL["resid_over"]
    t[k, j, i] = np.nextafter(HALF, f32(1))
    t, w = t.ravel(), w.ravel()
    t.setflags(write=False)
    w.setflags(write=False)
    return cfg, (t, w), fs.grid_of(cfg)


def exact_params(**kw):
    cfg, _, _ = exact_world()
    kw.setdefault("min_range_m", MIN_RANGE)
    kw.setdefault("max_range_m", MAX_RANGE)
    kw.setdefault("min_pairs", 0)
    return sts.params(cfg.trunc_margin, **kw)


def good_points(n, seed=5):
    """n points that all make pairs under exact_params(): seeded directions at ranges 0.55 ... 0.8, clear of the prepared
    cells (which lie at x >= 0.6 with y or z >= 0.2: these have x < 0.5)."""
    rng = np.random.default_rng(seed)
    out = np.zeros((0, 4), f32)
    while len(out) < n:
        d = rng.normal(size=(2 * n + 16, 3))
        d /= np.linalg.norm(d, axis=1, keepdims=True)
        p = d * rng.uniform(0.55, 0.8, (len(d), 1))
        p = p[p[:, 0] < 0.5]
        q = np.zeros((len(p), 4), f32)
        q[:, :3] = p
        out = np.concatenate([out, q])
    return out[:n].copy()


def centre(name):
    i, j, k = SPECIAL[name]
    return at(i + 0.5, j + 0.5, k + 0.5)


class SystemCase:
    """One tsdf_scan_track_system call at level 0 ... and the restatement's answer to it.  gate, special: the gate the case is
    named for and the indices of the points that must meet it (None: the points must be pairs)."""

    def __init__(self, name, points, P=None, flags=None, gate=None, special=(), world=None, pose=None):
        self.name = name
        self.cfg, self.vol, self.grid = exact_world() if world is None else world
        self.points = np.ascontiguousarray(points, f32).reshape(-1, 4)
        self.points.setflags(write=False)
        self.P = exact_params() if P is None else P
        self.flags = None if flags is None else np.ascontiguousarray(flags, np.uint8)
        self.gate, self.special = gate, tuple(special)
        self.pose = np.eye(4, dtype=f32).ravel() if pose is None else np.asarray(pose, f32).ravel()
        self._terms = {}

    def terms(self, level=0, info=None, scalar=False):
        key = (level, scalar)
        if key not in self._terms:
            M = sts.start_pose(self.grid, self.pose)
            i = {}
            fn = sts.pair_terms_scalar if scalar else sts.pair_terms
            t = fn(self.vol, self.grid, self.points, self.flags, M[:, :3].astype(f32), M[:, 3].astype(f32), level, self.P, i)
            t.setflags(write=False)
            self._terms[key] = (t, i)
        t, i = self._terms[key]
        if info is not None:
            info.update(i)
        return t

    def want(self, level=0):
        """(sums [29], bound [29]): n * 2^-52 * sum |term| for two double sums of the same terms (tests/align_cases.ts_bound)."""
        t = self.terms(level).astype(np.float64).reshape(-1, sts.N_TERMS)
        return t.sum(axis=0), t.shape[0] * 2.0 ** -52 * np.abs(t).sum(axis=0)

    def __repr__(self):
        return self.name


def with_points(extra, n_good=70):
    """good points with `extra` ([x, y, z] rows) put at even indices 8, 12, ... (multiples of 4: selected at every level);
    returns (points, the indices of the extra ones)."""
    pts = good_points(n_good)
    idx = [8 + 4 * k for k in range(len(extra))]
    for i, p in zip(idx, extra):
        pts[i, :3] = np.asarray(p, f32)
    return pts, idx


def _case(name, extra, gate, P=None, flags_on=False):
    pts, idx = with_points(extra)
    flags = None
    if flags_on:
        flags = np.zeros(len(pts), np.uint8)
        flags[idx] = 1
        flags[3] = 2                        # another flag value drops nothing
    return SystemCase(name, pts, P=P, flags=flags, gate=gate, special=idx)


COUNTS = (0, 1, 63, 64, 65, 257, 65601)


@functools.lru_cache(maxsize=None)
def count_case(n):
    """n points.  Up to 257 all of them make pairs; 65 601 (more than 256 x 256 lanes, so the grid-stride loop wraps): one
    point in 97 makes a pair, the rest are out of range, and the last 65 -- the wrapped lanes -- all make pairs."""
    if n <= 257:
        return SystemCase(f"{n} points", good_points(n, seed=7))
    pts = np.zeros((n, 4), f32)
    pts[:, 0] = 5.0
    live = np.flatnonzero((np.arange(n) % 97 == 0) | (np.arange(n) >= n - 65))
    pts[live] = good_points(len(live), seed=9)
    return SystemCase(f"{n} points, the last 65 beyond 256 x 256 lanes", pts)


@functools.lru_cache(maxsize=None)
def named_cases():
    below_min, above_one = np.nextafter(f32(MIN_RANGE), f32(0)), np.nextafter(f32(1), f32(2))
    rthr = float(HALF * f32(exact_world()[0].trunc_margin))
    i, j, k = SPECIAL["resid_on"]
    i2, j2, k2 = SPECIAL["resid_over"]
    out = [
        _case("a NaN coordinate", [[np.nan, 0.3, 0.2], [0.3, np.nan, 0.2], [0.3, 0.2, np.nan]], "finite"),
        _case("an infinite coordinate", [[np.inf, 0.3, 0.2], [0.3, -np.inf, 0.2]], "finite"),
        _case("range exactly at min_range_m", [[MIN_RANGE, 0, 0], [0, -MIN_RANGE, 0], [0, 0, MIN_RANGE]], None),
        _case("range exactly at max_range_m", [[0.5, 1.0, 1.0], [-0.5, 1.0, -1.0]], None),       # 0.25 + 1 + 1 = 1.5^2, exact
        _case("range one ulp outside", [[below_min, 0, 0], [0.5, above_one, 1.0]], "range"),
        _case("a flagged point", [[0.3, 0.4, 0.5]], "flag", P=exact_params(drop_flag=1), flags_on=True),
        _case("flags given, drop_flag -1", [[0.3, 0.4, 0.5]], None, flags_on=True),
        _case("g exactly 0", [at(0, 20, 20), at(20, 0, 20), at(20, 20, 0)], None),
        _case("g exactly dim - 1", [at(47, 20, 20), at(20, 47, 20), at(20, 20, 47)], "box", P=exact_params(max_range_m=3.0)),
        _case("a coordinate of 1e30, out of range", [[1e30, 0, 0], [0, -1e30, 0]], "range"),
        _case("a coordinate of 1e30 under a max_range_m whose square overflows", [[1e30, 0, 0], [0, -1e30, 0], [0, 0, 3e38]], "box",
              P=exact_params(max_range_m=3e38)),
        _case("a corner weight exactly at weight_thresh", [centre("weight")], "corner"),
        _case("|F| >= 1", [centre("free")], "band"),
        _case("|r| == resid_thresh", [at(i, j, k)], None, P=exact_params(resid_thresh=rthr)),
        _case("|r| the next float after resid_thresh", [at(i2, j2, k2)], "resid", P=exact_params(resid_thresh=rthr)),
        _case("a flat field with zero gradient", [centre("flat")], "normal"),
        SystemCase("n_points not a multiple of the stride", good_points(67, seed=8)),
    ]
    return out + [count_case(n) for n in COUNTS]


def system_vector(out29):
    return np.asarray(out29, np.float64).ravel()
