"""The parity cases of tests/test_gpu_extent.py (test infrastructure): grid shapes, uploaded states, the frames of the fused
state and the parameter sets, with the restatement's inputs computed once per case and shared.  tests/test_extent_spec.py
checks on the CPU, with the restatement alone, that no case is vacuous."""
import functools

import numpy as np

from semantic_slam_amd import capi, synth

f32 = np.float32
IM_HW = (120, 160)
K_SMALL = synth.TUM_K.copy()
K_SMALL[[0, 2, 4, 5]] *= 0.25          # the TUM camera at a quarter of its resolution
# a row of 5 quads (no multiple of the 8 quads a wavefront holds per row); one aligned wavefront row; partial workgroups in
# every axis; a row longer than a workgroup's x tile; and rows that are no multiple of 4 voxels (the per-voxel path), odd in
# every axis.  Then the shapes with more than the 32 wavefront tiles (32 x 8 voxels) a workgroup takes per slice, uploaded
# states only: 3 x 11 = 33 tiles of aligned rows (the second workgroup holds one tile and three wavefronts without any), 3 x 12 =
# 36 tiles of rows of 67 voxels (the per-voxel path), and rows of 66 000 voxels (65 workgroups per slice; x and x * x beyond
# 16 and 32 bits)
SHAPES = [(20, 12, 9), (64, 8, 5), (72, 33, 17), (260, 4, 3), (37, 22, 13), (96, 88, 3), (67, 93, 3), (66000, 4, 2)]
STATES = ["random", "edges", "fused"]
BANDS = [1.0, 0.25]
WEIGHT_THRESH = 0.9
VS = 0.004
N_FRAMES = 4
# The fused state per shape: (truncation in voxels, voxels by which the scene's back wall sits inside the grid's far face).
# Chosen with the restatement so that no case is vacuous (tests/test_extent_spec.py): in the thin grids the default band of
# five voxels covers every slice (no observed free space) and a wall on the far face leaves a band of 0.25 nearly empty.
FUSED = {(20, 12, 9): (5, 0.0), (64, 8, 5): (5, 0.0), (72, 33, 17): (8, 3.0), (260, 4, 3): (2, 0.7),
         (37, 22, 13): (5, 2.0)}



def states_of(dims):
    """The states a shape is tested in: the fused one only where FUSED has its scene."""
    return [s for s in STATES if s != "fused" or tuple(dims) in FUSED]


def workgroups_per_slice(dims):
    """csrc/tsdf_extent_host.hip.h, extent_blocks: wavefront tiles of 32 x 8 voxels, 32 of them per workgroup."""
    tiles = ((dims[0] + 3) // 4 + 7) // 8 * ((dims[1] + 7) // 8)
    return max(1, (tiles + 31) // 32)


ONE_BELOW = np.nextafter(f32(1), f32(0))
EDGE_T = np.array([0.0, -0.0, 1.0, -1.0, ONE_BELOW, -ONE_BELOW, np.nan, np.inf, -np.inf], f32)
EDGE_W = np.array([f32(0.9), np.nextafter(f32(0.9), f32(1)), np.nan], f32)


def margins(dims):
    """0 (no face counts), 1, and one larger than a dim (every surface voxel is near both faces of that axis)."""
    return [0, 1, min(dims) + 2]


def config(dims, origin=None, z_begin=0, z_end=None):
    origin = origin_of(dims) if origin is None else origin
    return capi.make_config(dims, VS, origin, trunc=trunc_of(dims), K=K_SMALL, im_height=IM_HW[0], im_width=IM_HW[1], z_begin=z_begin, z_end=z_end)


def origin_of(dims):
    """The grid centred on the optical axis, its near face 0.9 m in front of the base camera."""
    return np.array([-dims[0] * VS / 2, -dims[1] * VS / 2, 0.9], f32)


def trunc_of(dims):
    return float(f32(VS) * f32(FUSED[tuple(dims)][0])) if tuple(dims) in FUSED else None


def random_state(rng, n, p_fresh=0.2):
    """Values inside the band and weights above the threshold, 20 % of the voxels fresh (1, 0), 3 % observed free space (t = 1)
    and 3 % seen once with a weight at the threshold."""
    t = rng.uniform(-1.0, 1.0, n).astype(f32)
    w = rng.choice(np.array([1.0, 2.0, 3.0, 7.0], f32), n)
    u = rng.uniform(0, 1, n)
    t[u < p_fresh], w[u < p_fresh] = 1.0, 0.0
    t[(u >= p_fresh) & (u < p_fresh + 0.03)] = 1.0
    w[(u >= p_fresh + 0.03) & (u < p_fresh + 0.06)] = f32(0.9)
    return t, w


def edge_state(rng, n):
    """Half of the TSDF values and a third of the weights from the edge lists (every pair of them occurs), the rest ordinary."""
    t = rng.uniform(-1.2, 1.2, n).astype(f32)
    w = rng.choice(np.array([0.0, 1.0, 2.0, 3.0], f32), n, p=[0.1, 0.3, 0.3, 0.3])
    pick_t, pick_w = rng.uniform(0, 1, n) < 0.5, rng.uniform(0, 1, n) < 0.34
    t[pick_t] = rng.choice(EDGE_T, int(pick_t.sum()))
    w[pick_w] = rng.choice(EDGE_W, int(pick_w.sum()))
    k = 0                                  # every pair of the two lists, where both arrays take an edge value anyway
    for tv in EDGE_T:
        for wv in EDGE_W:
            t[k], w[k] = tv, wv
            k += 7
    return t, w


def frames(dims):
    """The four frames of the fused state: (poses [4, 16], depths [4, H, W]) of synth.SurfScene in the case's grid."""
    scene_origin = origin_of(dims) - np.array([0.0, 0.0, FUSED[tuple(dims)][1] * VS], f32)
    scene = synth.SurfScene(dims, VS, scene_origin, K=K_SMALL, h=IM_HW[0], w=IM_HW[1])
    poses = [scene.pose(k, n=8) for k in range(N_FRAMES)]
    return np.stack(poses), np.stack([scene.depth(c, quantize=True) for c in poses])


@functools.lru_cache(maxsize=None)
def state(dims, name):
    """(tsdf, weight) of the whole grid, read-only; the fused state through the CPU oracle (the device's Integrate is checked
    against it bit for bit elsewhere; tests/test_gpu_extent.py applies the restatement to what the device holds)."""
    n = int(np.prod(dims))
    rng = np.random.default_rng(sum(dims) + 31 * STATES.index(name))
    if name == "random":
        t, w = random_state(rng, n)
    elif name == "edges":
        t, w = edge_state(rng, n)
    else:
        from oracle.oracle import Oracle
        oracle = Oracle()
        cfg = config(dims)
        t, w = oracle.init_grid(dims)
        poses, depths = frames(dims)
        for c2w, d in zip(poses, depths):
            oracle.integrate(K_SMALL, oracle.cam2base(np.eye(4, dtype=f32).ravel(), c2w), d, dims, origin_of(dims), VS,
                             cfg.trunc_margin, t, w)
    t.setflags(write=False)
    w.setflags(write=False)
    return t, w


def params(band=1.0, margin=0, thr=WEIGHT_THRESH):
    p = capi.ExtentParams()
    p.weight_thresh, p.band, p.margin = thr, band, margin
    return p
