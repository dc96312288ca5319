"""The cases of tests/test_gpu_align.py (test infrastructure), shared with tests/test_align_spec.py, which checks on the CPU
that none of them is vacuous and that the tracked ones keep clear of the restatement's own thresholds.  Everything here is
computed once per case and handed out read-only.

Grids.  Destinations are fuse_cases.DST_SHAPES at 4 mm, truncation 20 mm, base frame = world.  Sources: fuse_cases.SRC_SHAPE
(24, 33, 17) at 5 mm for the two small destinations and LARGE_SRC (52, 42, 34) at 5 mm, which contains the (64, 48, 40)
destination's scene (its corners leave the box under the rotations), for that one; truncation 25 mm (ratio 1.25) or, for
pose 1, 15 mm (ratio 0.75); the source's box is centred on the destination's and moved by fuse_cases' seeded rigid transforms.
(In the system cases the large pair truncates at 32 and 40 / 24 mm: configs.)

States.  "surf": one scene sized by the DESTINATION's box (synth.SurfScene: the wall at its far face, so that a third of a
thin destination lies in the wall's band -- with fuse_cases' scene, sized by the source, under 13 % of a destination is a
candidate at all) fused into both grids through the CPU oracle, the source from four views (and 2 % of its voxels put back
to unobserved, as dropouts leave them), the destination from two of them with the right 45 % of the image missing (the large
one: all four, 8 %).  "edges": fuse_cases.edge_states (NaN, +-inf, +-0, +-1, weights at the threshold and one ulp above it),
with 8 % of the source's values replaced by +-4 so that a sample can leave the band at ratio 0.75 too.

One arithmetic fact limits the conditions: a source fused by Integrate holds values in [-1, 1], so at ratio 0.75 a sample
has |t| <= 0.75 and the band gate cannot reject; the "surf" cases of pose 1 must have that class EMPTY, and have."""
import functools
import math

import numpy as np

import align_spec as asp
import fuse_cases as fc
import fuse_spec as fs
import track_spec as ts
from semantic_slam_amd import capi, synth

f32 = np.float32
DST_SHAPES = fc.DST_SHAPES
BIG = (64, 48, 40)
LARGE_SRC = (52, 42, 34)
LEVELS = (0, 1, 2)
STATES = fc.STATES
N_POSES = fc.N_POSES
RESID = {"surf": 0.25, "edges": 1.0}        # resid_thresh of the system cases: both sides of it occur in either state
MAX_BLOCKS, TILE_X, TILE_Y = 256, 16, 4     # csrc/tsdf_align.hip.h: kAlignMaxBlocks and the wavefront's lattice tile


def src_shape(dst_dims):
    return LARGE_SRC if tuple(dst_dims) == BIG else fc.SRC_SHAPE


def configs(dst_dims, pose, thick=True):
    """fuse_cases.configs' recipe with the source shape of this destination (the same seeds, rotations and shifts).  thick:
    the large destination truncates at 32 mm and its source at 40 or 24 mm (the same ratios): with the default 20 mm band the
    surfaces of one sphere and one wall put under 10 % of a 256 x 192 x 160 mm box near a surface of both volumes."""
    shape = src_shape(dst_dims)
    if shape == fc.SRC_SHAPE:
        return fc.configs(dst_dims, pose)
    d_ext, s_ext = np.array(dst_dims) * fc.DST_VS, np.array(shape) * fc.SRC_VS
    centre = np.array([0.0, 0.0, 0.9 + d_ext[2] / 2])
    rng = np.random.default_rng(100 + pose)
    ax, ay, az = rng.uniform(-0.25, 0.25, 3)
    R = synth.rot_z(az) @ synth.rot_y(ay) @ synth.rot_x(ax)
    shift = rng.uniform(-0.004, 0.004, 3) + (np.array([0.03, 0.02, 0.01]) if pose == 2 else 0.0)
    d_trunc = 0.032 if thick else 0.020
    s_trunc = d_trunc * (0.75 if pose == 1 else 1.25)
    return (fc.config(dst_dims, fc.DST_VS, (centre - d_ext / 2).astype(f32), trunc=d_trunc),
            fc.config(shape, fc.SRC_VS, (centre - s_ext / 2).astype(f32), trunc=s_trunc, base2world=fs.pose_about(R, centre, shift)))


def centre_of(cfg):
    return np.asarray(cfg.origin, np.float64) + np.array([cfg.dim_x, cfg.dim_y, cfg.dim_z]) * float(cfg.voxel_size) / 2


def moved(dst2src, centre, deg, metres, seed):
    """dst2src with a seeded rigid motion of the destination's frame in front of it: a rotation of `deg` about a random axis
    through `centre` and a shift of `metres` in a random direction (float64, rounded to float32 [16])."""
    rng = np.random.default_rng(seed)
    ax, d = rng.normal(size=3), rng.normal(size=3)
    R = ts.rodrigues(ax / np.linalg.norm(ax) * math.radians(deg))
    T = fs.pose_about(R, centre, d / np.linalg.norm(d) * metres).astype(np.float64).reshape(4, 4)
    return (np.asarray(dst2src, np.float64).reshape(4, 4) @ T).astype(f32).ravel()


def fuse_views(oracle, scene, cfg, views, part=None):
    """The scene's quantised depth from `views` fused into cfg's grid through the CPU oracle; part: the image columns kept."""
    dims, origin, vs, trunc, b2w = fs.grid_of(cfg)
    t, w = oracle.init_grid(dims)
    for c2w in views:
        depth = scene.depth(c2w, quantize=True)
        if part is not None:
            depth = depth.copy()
            depth[:, part:] = 0.0
        oracle.integrate(fc.K_SMALL, oracle.cam2base(b2w, c2w), depth, dims, origin, float(vs), float(trunc), t, w)
    return t, w


@functools.lru_cache(maxsize=None)
def states(dst_dims, pose, state):
    """(dst cfg, src cfg, (dst t, dst w, src t, src w)), read-only."""
    from oracle.oracle import Oracle
    dcfg, scfg = configs(dst_dims, pose)
    n_dst, n_src = int(np.prod(dst_dims)), int(np.prod(src_shape(dst_dims)))
    if state == "surf":
        orc = Oracle()
        scene = synth.SurfScene(dst_dims, fc.DST_VS, np.asarray(dcfg.origin, f32), K=fc.K_SMALL, h=fc.IM_HW[0], w=fc.IM_HW[1])
        views = [scene.pose(k, n=8) for k in range(4)]
        st, sw = fuse_views(orc, scene, scfg, views)
        holes = np.random.default_rng(300 + pose).uniform(0, 1, n_src) < 0.02      # dropouts: a corner that was never observed
        st[holes], sw[holes] = 1.0, 0.0
        big = tuple(dst_dims) == BIG
        dt, dw = fuse_views(orc, scene, dcfg, views[:4 if big else 2], part=int((0.92 if big else 0.55) * fc.IM_HW[1]))
    else:
        seed = 7 * pose + len(dst_dims) + dst_dims[0]
        dt, dw, st, sw = fc.edge_states(seed, n_dst, n_src)
        rng = np.random.default_rng(1000 + seed)
        far = rng.uniform(0, 1, n_src) < 0.08
        st[far] = rng.choice(np.array([4.0, -4.0], f32), int(far.sum()))
    arrays = (dt, dw, st, sw)
    for a in arrays:
        a.setflags(write=False)
    return dcfg, scfg, arrays


def align_params(P):
    """The capi.AlignParams of a spec dict."""
    p = capi.AlignParams()
    p.weight_thresh, p.resid_thresh, p.n_levels = float(P["weight_thresh"]), float(P["resid_thresh"]), P["n_levels"]
    p.iters[:] = list(P["iters"])
    p.min_pairs, p.eps_rot, p.eps_trans = P["min_pairs"], P["eps_rot"], P["eps_trans"]
    return p


class SystemCase:
    """One tsdf_align_system call and the restatement's answer to it."""

    def __init__(self, name, dcfg, scfg, arrays, dst2src, level, P):
        self.name, self.dcfg, self.scfg, self.arrays, self.level, self.P = name, dcfg, scfg, arrays, level, P
        self.dst2src = np.asarray(dst2src, f32).ravel()
        self.grids = (fs.grid_of(dcfg), fs.grid_of(scfg))
        self.info = {}
        M = asp.start_pose(self.grids, self.dst2src)
        self.terms = asp.pair_terms(arrays[:2], arrays[2:], self.grids, M[:, :3].astype(f32), M[:, 3].astype(f32), level, P,
                                    self.info)
        self.terms.setflags(write=False)

    def want(self):
        return ts_bound(self.terms)

    def __repr__(self):
        return self.name


def ts_bound(terms):
    """(sums [29], bound [29]): track_cases.system_bound's n * 2^-52 * sum |term| for two double sums of the same terms."""
    t = np.asarray(terms, f32).astype(np.float64).reshape(-1, asp.N_TERMS)
    return t.sum(axis=0), t.shape[0] * 2.0 ** -52 * np.abs(t).sum(axis=0)


def system_vector(A, b, r2, n):
    """Volume.align_system's answer as the 29 values."""
    return np.concatenate([np.asarray(A)[np.triu_indices(6)], b, [r2, float(n)]])


@functools.lru_cache(maxsize=None)
def parity_case(dst_dims, pose, state, level):
    """The system at the pose the two base2world give, moved by 0.5 deg / 2 mm about the destination's centre so that the
    residuals are those of two surfaces that do not quite coincide."""
    dcfg, scfg, arrays = states(dst_dims, pose, state)
    P = asp.params(resid_thresh=RESID[state], n_levels=3)
    grids = (fs.grid_of(dcfg), fs.grid_of(scfg))
    pose16 = moved(asp.pose_default(grids), centre_of(dcfg), 0.5, 0.002, 200 + pose)
    return SystemCase(f"{'x'.join(map(str, dst_dims))} pose {pose} {state} level {level}", dcfg, scfg, arrays, pose16, level, P)


def parity_keys():
    return [(d, p, s, l) for d in DST_SHAPES for p in range(N_POSES) for s in STATES for l in LEVELS]


# ------------------------------------------------------------------------------------------------------------------------
# where a lattice point sits in the kernel's walk (the MAPPING of csrc/tsdf_align.hip.h), the uploaded states that pick points
# ------------------------------------------------------------------------------------------------------------------------
def device_lanes(dims, level):
    """(lane index of every lattice point in asp.lattice's order, workgroups of the launch, lanes of the launch): a wavefront
    takes a TILE_X x TILE_Y tile of one lattice slice, tiles x fastest, then y, then z; lane index = tile * 64 + lane."""
    s = 1 << level
    ln = [-(-d // s) for d in dims]
    tx, ty = -(-ln[0] // TILE_X), -(-ln[1] // TILE_Y)
    lz, ly, lx = [a.ravel() for a in np.meshgrid(np.arange(ln[2]), np.arange(ln[1]), np.arange(ln[0]), indexing="ij")]
    tile = (lz * ty + ly // TILE_Y) * tx + lx // TILE_X
    lanes = tx * ty * ln[2] * 64
    return tile * 64 + (ly % TILE_Y) * TILE_X + lx % TILE_X, max(1, min(-(-lanes // 256), MAX_BLOCKS)), lanes


EXACT_VS = 2.0 ** -8        # a power of two, origins multiples of it: positions and grid coordinates are exact
EXACT_COUNTS = (1, 63, 64, 65, 255, 256, 257)


@functools.lru_cache(maxsize=None)
def exact_grids():
    """The (64, 48, 40) destination and a source that is the same grid shifted by (3.25, 2.5, 1.75) voxels and two voxels
    larger on every side, identity base2world, equal truncations: every destination voxel lies in a source cell, with
    fractions (0.25, 0.5, 0.75)."""
    ddims, sdims = BIG, (72, 56, 48)
    do = np.array([-32 * EXACT_VS, -24 * EXACT_VS, 230 * EXACT_VS], f32)
    so = do - np.array([3.25, 2.5, 1.75], f32) * f32(EXACT_VS)
    trunc = float(f32(EXACT_VS) * f32(5))
    return fc.config(ddims, EXACT_VS, do, trunc=trunc), fc.config(sdims, EXACT_VS, so, trunc=trunc)


@functools.lru_cache(maxsize=None)
def exact_source():
    """A smooth source field, fully observed: a plane's signed distance in truncation units with a gentle ripple, |values| < 0.9."""
    _, scfg = exact_grids()
    z, y, x = np.meshgrid(*[np.arange(d, dtype=np.float64) for d in (scfg.dim_z, scfg.dim_y, scfg.dim_x)], indexing="ij")
    t = 0.05 * (x - 36) / 5 + 0.03 * (y - 28) / 5 - 0.04 * (z - 24) / 5 + 0.05 * np.sin(0.3 * x + 0.2 * y + 0.25 * z)
    t = t.astype(f32).ravel()
    assert np.abs(t).max() < 0.9
    w = np.full(t.size, 2.0, f32)
    t.setflags(write=False)
    w.setflags(write=False)
    return t, w


def picked_case(name, picks, level=0):
    """A destination whose only candidates are the lattice points `picks` (indices in asp.lattice's order): weight 2 and a
    TSDF of 0.05 there, (1, 0) everywhere else."""
    dcfg, scfg = exact_grids()
    (x0, x1, x2), _, _ = asp.lattice(BIG, level)
    picks = np.asarray(picks, np.int64)
    at = (x2[picks] * BIG[1] + x1[picks]) * BIG[0] + x0[picks]
    dt, dw = np.ones(int(np.prod(BIG)), f32), np.zeros(int(np.prod(BIG)), f32)
    dt[at], dw[at] = 0.05, 2.0
    st, sw = exact_source()
    grids = (fs.grid_of(dcfg), fs.grid_of(scfg))
    return SystemCase(name, dcfg, scfg, (dt, dw, st, sw), asp.pose_default(grids), level, asp.params(n_levels=3))


def interior_points(level=0, margin=0):
    """Lattice points (asp.lattice's order) at least `margin` voxels from every face of the (64, 48, 40) destination."""
    (x0, x1, x2), _, _ = asp.lattice(BIG, level)
    ok = np.ones(x0.size, bool)
    for x, d in zip((x0, x1, x2), BIG):
        ok &= (x >= margin) & (x < d - margin)
    return np.flatnonzero(ok)


@functools.lru_cache(maxsize=None)
def reduction_case(n):
    """Exactly n candidates, all of them pairs, spread over the interior of the lattice in the kernel's walk order: the
    first, the last, and the ones between at even steps of the lane index."""
    pts = interior_points()
    lane, _, _ = device_lanes(BIG, 0)
    pts = pts[np.argsort(lane[pts])]
    picks = pts[np.unique(np.linspace(0, pts.size - 1, n).astype(np.int64))]
    assert picks.size == n
    return picked_case(f"exactly {n} candidates", picks)


@functools.lru_cache(maxsize=None)
def last_trip_case():
    """Candidates only where the last workgroup makes its last trip through the grid-stride loop."""
    lane, blocks, lanes = device_lanes(BIG, 0)
    trips = -(-lanes // (blocks * 256))
    assert trips >= 2
    pts = interior_points()
    first = (trips - 1) * blocks * 256
    last_block_of_trip = (lanes - 1 - first) // 256          # the workgroup that takes the launch's last lanes
    sel = pts[(lane[pts] >= first + last_block_of_trip * 256)]
    assert sel.size >= 8
    return picked_case("the last workgroup's last trip", sel), first + last_block_of_trip * 256


# ------------------------------------------------------------------------------------------------------------------------
# whole runs: a scene without symmetry fused into both grids from different views, the source's pose perturbed
# ------------------------------------------------------------------------------------------------------------------------
TRACK_VIEWS = list(range(0, 64, 8))
# (rotation in degrees, translation in metres, seed) of the motion the source's base2world is off by, about the scene's centre;
# the last one lies outside the basin (the surfaces are several truncation distances, 20 mm, apart over most of the scene)
MAGNITUDES = [(1.0, 0.003, 31), (2.0, 0.006, 32), (4.0, 0.010, 33), (8.0, 0.020, 36), (30.0, 0.100, 34)]
INSIDE = MAGNITUDES[:4]


@functools.lru_cache(maxsize=None)
def run_world():
    """(dst cfg, src cfg as fused, (dst t, dst w, src t, src w), the true dst2src): synth.TrackScene in the (64, 48, 40)
    destination's box, the source LARGE_SRC at 5 mm under pose 0's rigid transform; the source is fused from all eight views
    of the orbit, the destination from every other one."""
    from oracle.oracle import Oracle
    dcfg, scfg = configs(BIG, 0, thick=False)
    orc = Oracle()
    scene = synth.TrackScene(BIG, fc.DST_VS, np.asarray(dcfg.origin, f32), K=fc.K_SMALL, h=fc.IM_HW[0], w=fc.IM_HW[1])
    views = [scene.pose(k) for k in TRACK_VIEWS]
    st, sw = fuse_views(orc, scene, scfg, views)
    dt, dw = fuse_views(orc, scene, dcfg, views[::2])
    arrays = (dt, dw, st, sw)
    for a in arrays:
        a.setflags(write=False)
    truth = asp.pose_default((fs.grid_of(dcfg), fs.grid_of(scfg)))
    return dcfg, scfg, arrays, truth


def perturbed_source(deg, metres, seed):
    """(src cfg whose base2world is off by the seeded motion, the dst2src it gives by default)."""
    dcfg, scfg, _, truth = run_world()
    start = moved(truth, centre_of(dcfg), deg, metres, seed)
    # base2world_src' with inverse(base2world_src') * base2world_dst = start; dst's base2world is the identity
    _, b2w = capi.invert_matrix(start)
    cfg = fc.config(LARGE_SRC, fc.SRC_VS, np.asarray(scfg.origin, f32), trunc=scfg.trunc_margin, base2world=b2w)
    return cfg, start


class RunCase:
    """One tsdf_align_volume call (guess: 16 float32 or None = the pose the two base2world give) and the restatement's run."""

    def __init__(self, name, dcfg, scfg, arrays, P, guess=None):
        self.name, self.dcfg, self.scfg, self.arrays, self.P = name, dcfg, scfg, arrays, P
        self.guess = None if guess is None else np.asarray(guess, f32).ravel()
        self.grids = (fs.grid_of(dcfg), fs.grid_of(scfg))
        self._want = None

    def want(self):
        if self._want is None:
            hist = []
            r = asp.align(self.arrays[:2], self.arrays[2:], self.grids, self.P, self.guess, hist)
            r["history"], r["rmse32"] = hist, f32(r["rmse"])
            self._want = r
        return self._want

    def __repr__(self):
        return self.name


def preconditions(history, P):
    """track_cases.preconditions (a step within 10 % of an eps, a pivot within a factor 2 of the lost threshold), and: a pair
    count within 1 of min_pairs is fine (integers), but a computed comparison within one float32 spacing of its threshold
    (asp.pair_terms' "near") is a breach."""
    import track_cases as tc
    bad = tc.preconditions(history, {"eps_rot": P["eps_rot"], "eps_trans": P["eps_trans"]})
    for k, h in enumerate(history):
        if any(h["near"].values()):
            bad.append((k, "near", h["near"]))
    return bad


ITERS = [(10, 10, 0), (0, 4, 0), (3, 0, 0), (0, 0, 2), (1, 1, 1), (0, 0, 0)]
# Every seed is the first one tried, except: of the 49 runs one, (n_levels, iters, eps) below, took a step with
# |tau| / eps_trans = 0.96 at seed 31 (a breach of preconditions) and was given the seed named here instead.
RESEEDED = {(2, (1, 1, 1), 1e-3): 41}


@functools.lru_cache(maxsize=None)
def state_machine_cases():
    dcfg, scfg, arrays, truth = run_world()
    out = []
    cfg1, start1 = perturbed_source(*MAGNITUDES[0])
    for n_levels in (1, 2, 3):
        for iters in ITERS:
            for eps in (1e-5, 1e-3):
                cfg1 = perturbed_source(1.0, 0.003, RESEEDED.get((n_levels, iters, eps), MAGNITUDES[0][2]))[0]
                out.append(RunCase(f"n_levels {n_levels} iters {iters} eps {eps}", dcfg, cfg1, arrays,
                                   asp.params(n_levels=n_levels, iters=iters, eps_rot=eps, eps_trans=eps, min_pairs=100)))
    for deg, metres, seed in MAGNITUDES:
        cfg, start = perturbed_source(deg, metres, seed)
        out.append(RunCase(f"default schedule from {deg} deg {1e3 * metres:.0f} mm", dcfg, cfg, arrays, asp.params()))
        out.append(RunCase(f"guess {deg} deg {1e3 * metres:.0f} mm", dcfg, scfg, arrays, asp.params(), guess=start))
    cfg1 = perturbed_source(*MAGNITUDES[0])[0]
    first = []
    asp.align(arrays[:2], arrays[2:], (fs.grid_of(dcfg), fs.grid_of(cfg1)), asp.params(n_levels=3, iters=(0, 0, 1)), None, first)
    c = first[0]["pairs"]
    out.append(RunCase(f"min_pairs c = {c}", dcfg, cfg1, arrays, asp.params(n_levels=3, iters=(10, 5, 1), min_pairs=c)))
    out.append(RunCase(f"min_pairs c + 1 = {c + 1}", dcfg, cfg1, arrays, asp.params(n_levels=3, iters=(10, 5, 1), min_pairs=c + 1)))
    out.append(RunCase("resid_thresh 1e-4: lost at level 0", dcfg, cfg1, arrays,
                       asp.params(n_levels=1, iters=(5, 0, 0), resid_thresh=1e-4)))
    return out


def empty_source_case(guess):
    """A source no frame has touched: lost in the first iteration of the first level that runs."""
    dcfg, scfg, arrays, truth = run_world()
    n = int(np.prod(LARGE_SRC))
    empty = (arrays[0], arrays[1], np.ones(n, f32), np.zeros(n, f32))
    return RunCase("an empty source", dcfg, scfg, empty, asp.params(n_levels=3, iters=(4, 0, 3)), guess=guess)


def band_ratio(counts):
    return counts["agree_band"] / counts["both_band"] if counts["both_band"] else 0.0
