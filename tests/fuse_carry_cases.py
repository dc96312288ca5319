"""The cases of tests/test_gpu_fuse_carry.py (test infrastructure): destination and source configurations (fuse_cases'),
states of all six arrays per side -- fused on the CPU through the oracle, or edge-valued -- and the two lattice cases, with
the restatement's result computed once per case and shared.  tests/test_fuse_carry_spec.py checks on the CPU that no case is
vacuous."""
import functools

import numpy as np

import fuse_cases as fc
import fuse_carry_spec as fcs
import fuse_spec as fs
from semantic_slam_amd import synth

f32 = np.float32
# 16-byte rows all (labels and colour need dim_x % 4 == 0); more than one workgroup per axis; last x tiles of 8, 3 and 1 quads;
# z extents that are no multiple of the z-run of 16 slices per workgroup
DST_SHAPES = [(64, 48, 40), (44, 12, 9), (36, 22, 13)]
N_POSES = 3
STATES = ["surf", "edges"]
CARRIES = [1, 2, 3]
PROB_THD = 0.5
VS = 2.0 ** -8                     # the lattice cases' voxel size (test_fuse_spec.lattice_shift_case)


def rgb_pattern(k):
    h, w = fc.IM_HW
    v, u = np.mgrid[0:h, 0:w]
    return np.stack([(3 * u + 40 * k) % 256, (5 * v + 17 * k) % 256, (2 * (u + v)) % 256], -1).astype(np.uint8)


def label_images(boundary, low_top):
    """Instance 1 left of the image column `boundary`, instance 2 from it on, no instance in the top 6 rows; the score is 0.8,
    or with low_top 0.2 in the upper half and 0.9 in the lower."""
    h, w = fc.IM_HW
    lab = np.where(np.arange(w)[None, :] < boundary, 1, 2).astype(np.uint16) * np.ones((h, 1), np.uint16)
    lab[:6] = 0
    score = np.full((h, w), 0.8, f32)
    if low_top:
        score[:h // 2], score[h // 2:] = 0.2, 0.9
    return lab, score


def empty_attributes(n):
    return np.zeros(n, np.uint32), np.zeros(n, np.uint16), np.zeros(n, f32), np.zeros(n, f32)


def surf_states(oracle, dcfg, scfg):
    """fuse_cases.surf_states with colour and labels: the source from four views, the destination from two of them with the
    right 45 % of the image missing.  The instance boundary sits at 50 % of the image width in the source's label images and
    at 40 % in the destination's, so the voxels between the two are opposed; the source's scores are low in the upper half
    of the image (its votes lose there) and high in the lower half (they win)."""
    ddims, d_origin, d_vs, d_trunc, d_b2w = fs.grid_of(dcfg)
    sdims, s_origin, s_vs, s_trunc, s_b2w = fs.grid_of(scfg)
    K, (h, w) = fc.K_SMALL, fc.IM_HW
    scene = synth.SurfScene(sdims, float(s_vs), s_origin, K=K, h=h, w=w)
    dt, dw = oracle.init_grid(ddims)
    st, sw = oracle.init_grid(sdims)
    dcol, dlab, dfp, dbp = empty_attributes(dt.size)
    scol, slab, sfp, sbp = empty_attributes(st.size)
    s_lab, s_score = label_images(int(0.50 * w), True)
    d_lab, d_score = label_images(int(0.40 * w), False)
    for k in range(4):
        c2w = scene.pose(k, n=8)
        depth = scene.depth(c2w, quantize=True)
        rgb = rgb_pattern(k)
        c2b = oracle.cam2base(s_b2w, c2w)
        grid = (sdims, s_origin, float(s_vs), float(s_trunc))
        oracle.integrate(K, c2b, depth, *grid, st, sw)
        oracle.integrate_colour(K, c2b, depth, rgb, *grid, sw, scol)
        oracle.integrate_labels(K, c2b, depth, s_lab, s_score, *grid, slab, sfp, sbp, prob_thd=PROB_THD)
        if k < 2:
            part = depth.copy()
            part[:, int(0.55 * w):] = 0.0
            c2b = oracle.cam2base(d_b2w, c2w)
            grid = (ddims, d_origin, float(d_vs), float(d_trunc))
            oracle.integrate(K, c2b, part, *grid, dt, dw)
            oracle.integrate_colour(K, c2b, part, rgb, *grid, dw, dcol)
            oracle.integrate_labels(K, c2b, part, d_lab, d_score, *grid, dlab, dfp, dbp, prob_thd=PROB_THD)
    return (dt, dw, dcol, dlab, dfp, dbp), (st, sw, scol, slab, sfp, sbp)


def edge_attributes(rng, n):
    """Random packed colours (top byte 0) with 10 % of each channel pure 255; labels 0..3; Fp / Bp uniform, 30 % of them from
    {0.5, 1, 1.5, 2} (sums of these meet the threshold exactly: equal evidence) and 8 % NaN, +-inf or 0."""
    col = rng.integers(0, 1 << 24, n, dtype=np.uint32)
    for s in (0, 8, 16):
        col[rng.uniform(0, 1, n) < 0.10] |= np.uint32(255 << s)
    lab = rng.integers(0, 4, n).astype(np.uint16)
    out = [col, lab]
    for _ in range(2):
        a = rng.uniform(0.05, 3.0, n).astype(f32)
        pick = rng.uniform(0, 1, n) < 0.30
        a[pick] = rng.choice(np.array([0.5, 1.0, 1.5, 2.0], f32), int(pick.sum()))
        pick = rng.uniform(0, 1, n) < 0.08
        a[pick] = rng.choice(np.array([np.nan, np.inf, -np.inf, 0.0], f32), int(pick.sum()))
        out.append(a)
    return tuple(out)


def edge_states(seed, n_dst, n_src):
    dt, dw, st, sw = fc.edge_states(seed, n_dst, n_src)
    rng = np.random.default_rng(1000 + seed)
    return (dt, dw) + edge_attributes(rng, n_dst), (st, sw) + edge_attributes(rng, n_src)


@functools.lru_cache(maxsize=None)
def states(dst_dims, pose, state):
    """(dst cfg, src cfg, the destination's six arrays, the source's six) -- computed once, not to be changed by its users."""
    from oracle.oracle import Oracle
    dcfg, scfg = fc.configs(dst_dims, pose)
    if state == "surf":
        dst, src = surf_states(Oracle(), dcfg, scfg)
    else:
        dst, src = edge_states(7 * pose + len(dst_dims) + dst_dims[0], int(np.prod(dst_dims)), int(np.prod(fc.SRC_SHAPE)))
    for a in dst + src:
        a.setflags(write=False)
    return dcfg, scfg, dst, src


@functools.lru_cache(maxsize=None)
def parity_case(dst_dims, pose, state, carry, write=1):
    """(dst cfg, src cfg, dst arrays, src arrays, the six arrays wanted, the eight counts wanted, info)."""
    dcfg, scfg, dst, src = states(dst_dims, pose, state)
    info = {}
    want, counts = fcs.fuse_carry(dst, fs.grid_of(dcfg), src, fs.grid_of(scfg), carry, prob_thd=PROB_THD,
                                  weight_thresh=fc.WEIGHT_THRESH, agree_tol=0.4, write=write, info=info)
    for a in want:
        a.setflags(write=False)
    return dcfg, scfg, dst, src, want, counts, info


# ------------------------------------------------------------------------------------------------------------------------
# the lattice cases: voxel size 2^-8, origins at multiples of half of it, so every position and fraction is exact
# ------------------------------------------------------------------------------------------------------------------------
def lattice_grid(dims, origin):
    return (tuple(dims), np.asarray(origin, f32), f32(VS), f32(VS) * f32(5), np.eye(4, dtype=f32).ravel())


def lattice_source(seed, sdims, x_only_red=False):
    """A source every voxel of which is observed (weight 2, TSDF inside the band) and labelled 1..3 with positive evidence;
    with x_only_red the red channel depends on x alone, so a mean over the cell is a mean of two values."""
    rng = np.random.default_rng(seed)
    n = int(np.prod(sdims))
    t = rng.uniform(-0.9, 0.9, n).astype(f32)
    w = np.full(n, 2.0, f32)
    col = rng.integers(0, 1 << 24, n, dtype=np.uint32)
    if x_only_red:
        red = rng.integers(0, 256, sdims[0], dtype=np.uint32)
        col = (col & np.uint32(0xFFFF00)) | np.tile(red, sdims[1] * sdims[2])
    lab = rng.integers(1, 4, n).astype(np.uint16)
    fp = rng.uniform(0.1, 3.0, n).astype(f32)
    bp = rng.uniform(0.0, 3.0, n).astype(f32)
    return t, w, col, lab, fp, bp


def fresh(n):
    return (np.ones(n, f32), np.zeros(n, f32)) + empty_attributes(n)


@functools.lru_cache(maxsize=None)
def lattice_copy_case():
    """test_fuse_spec.lattice_shift_case with attributes: (dst grid, src grid, fresh dst, src, what the destination must hold:
    the source's bits in the shifted block where the merge takes the voxel over, zeros elsewhere; voxels taken over)."""
    from test_fuse_spec import lattice_shift_case
    dg, sg, t, w, want_t, want_w, taken = lattice_shift_case()
    sdims, ddims = sg[0], dg[0]
    rng = np.random.default_rng(11)
    _, _, col, lab, fp, bp = lattice_source(12, sdims)
    lab[rng.uniform(0, 1, lab.size) < 0.1] = 0          # no instance: nothing to carry, and no evidence either
    fp[lab == 0], bp[lab == 0] = 0.0, 0.0
    box = (slice(0, sdims[2]), slice(4, 4 + sdims[1]), slice(8, 8 + sdims[0]))      # z, y, x
    take = ((w > f32(0.9)) & (t > f32(-1))).reshape(sdims[::-1])
    want = [want_t, want_w]
    for a in (col, lab, fp, bp):
        full = np.zeros(ddims[::-1], a.dtype)
        full[box] = np.where(take, a.reshape(sdims[::-1]), 0)
        want.append(full.ravel())
    return dg, sg, fresh(want_t.size), (t, w, col, lab, fp, bp), tuple(want), taken


@functools.lru_cache(maxsize=None)
def half_voxel_case():
    """A fresh destination whose voxel centres sit half a voxel off the source's lattice on every axis (f == 0.5): the
    nearest corner is the upper one, and colour means land on halves.  (dst grid, src grid, fresh dst, src)."""
    sdims, ddims = (24, 18, 10), (40, 30, 13)
    so = np.array([-12 * VS, -9 * VS, 230 * VS], f32)
    do = so - np.array([8.5 * VS, 4.5 * VS, 0.5 * VS], f32)
    return lattice_grid(ddims, do), lattice_grid(sdims, so), fresh(int(np.prod(ddims))), lattice_source(13, sdims, x_only_red=True)
