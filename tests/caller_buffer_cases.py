"""The cases of tests/test_gpu_caller_buffers.py (test infrastructure, no GPU): image sizes at which a four-wide access
goes wrong, the walk's three volume shape classes, and a camera under which the FIRST and the LAST element of every caller
image is really consumed.  tests/test_caller_buffer_cases.py holds the cases to those conditions on the CPU, so that a later
edit here cannot hollow the GPU tests out.

Camera: on the volume's axis in front of its near face, identity pose; focal lengths such that the volume over-fills the image
by 1.3 at its far face (every pixel's ray runs through voxels); centre ((W-1)/2 + 0.2, (H-1)/2 - 0.3).  Depth: planes through
the volume's middle, tilted a little and differently per frame, so that rows, columns and frames all differ.
"""
import functools

import numpy as np

from semantic_slam_amd import capi
from walk_cases import CLASSES, origin_of

f32 = np.float32

# (H, W): H*W mod 4 = 1, 2, 3 with W odd, and one size with W % 4 == 0 where a vector path is legitimate at residue 0
SIZES = [(33, 45), (30, 41), (37, 51), (24, 32)]
VOLUMES = ["row", "flat", "scalar"]
OVERFILL = 1.3
N_FRAMES = 3
K_MASKS = 3
EYE = np.eye(4, dtype=f32).ravel()
PAIRS = [(hw, cls) for hw in SIZES for cls in VOLUMES]


def pair_id(pair):
    (h, w), cls = pair
    return f"{h}x{w}-{cls}"


def four_wide(cls):
    """Labels, colour and batches refuse rows that are no multiple of 4 voxels."""
    return CLASSES[cls]["dims"][0] % 4 == 0


class Case:
    pass


@functools.lru_cache(maxsize=None)
def case(hw, cls):
    """Everything a test of one (image size, shape class) pair feeds the library; arrays are shared and read-only."""
    h, w = hw
    c = Case()
    c.hw, c.cls = hw, cls
    c.dims, c.vs = CLASSES[cls]["dims"], CLASSES[cls]["vs"]
    c.origin = origin_of(c.dims, c.vs)
    depth_extent = c.dims[2] * c.vs
    z_near, z_far = float(c.origin[2]), float(c.origin[2]) + depth_extent
    fx = OVERFILL * w * z_far / (c.dims[0] * c.vs)
    fy = OVERFILL * h * z_far / (c.dims[1] * c.vs)
    c.K = np.array([fx, 0, (w - 1) / 2 + 0.2, 0, fy, (h - 1) / 2 - 0.3, 0, 0, 1], f32)
    c.cfg = capi.make_config(c.dims, c.vs, c.origin, K=c.K, im_height=h, im_width=w)
    c.pose = EYE
    rng = np.random.default_rng([17, h, w, VOLUMES.index(cls)])
    z_mid = (z_near + z_far) / 2
    u, v = np.meshgrid((np.arange(w) - (w - 1) / 2) / w, (np.arange(h) - (h - 1) / 2) / h)
    tilts = [(0.30, -0.20), (-0.25, 0.35), (0.15, 0.30)]             # fractions of the volume's depth, corner to corner
    c.depths = [(z_mid + depth_extent * (a * u + b * v)).astype(f32) for a, b in tilts[:N_FRAMES]]
    c.raws = [np.round(d.astype(np.float64) * 5000.0).astype(np.uint16) for d in c.depths]
    c.median = float(np.median(c.depths[0]))
    # object_origin takes per-axis minima: frame 0 has its smallest x at the first pixel; the last pixel gets the smallest z
    c.origin_depth = c.depths[0].copy()
    c.origin_depth.flat[-1] = c.depths[0].min() - f32(0.01)
    # mask 0: clear on the first pixel, set on the last; mask 1 the reverse; mask 2 random with both set
    masks = [(rng.uniform(0, 1, hw) < 0.7).astype(np.uint8) * 255 for _ in range(K_MASKS)]
    masks[0].flat[0], masks[0].flat[-1] = 0, 255
    masks[1].flat[0], masks[1].flat[-1] = 255, 0
    masks[2].flat[0], masks[2].flat[-1] = 255, 255
    c.masks = masks
    # compose_labels' K images: the stack's first byte (mask 1, first pixel) and last byte (mask 0, last pixel) both belong to
    # the instance that wins its pixel under the scores below
    c.mask_stack = np.stack([masks[1], masks[2], masks[0]])
    c.rgb = rng.integers(0, 256, (h, w, 3)).astype(np.uint8)
    c.labels = np.array([7, 21, 40], np.uint16)                       # one label and score per instance mask (compose_labels)
    c.scores = np.array([0.9, 0.6, 0.8], f32)
    c.label_ims = [rng.integers(1, 50, hw).astype(np.uint16) for _ in range(N_FRAMES)]
    c.score_ims = [rng.uniform(0.3, 1.0, hw).astype(f32) for _ in range(N_FRAMES)]
    for arrs in (c.depths, c.raws, c.masks, c.label_ims, c.score_ims, [c.rgb, c.K, c.labels, c.scores, c.mask_stack, c.origin_depth]):
        for a in arrs:
            a.setflags(write=False)
    return c


def batch_configs(c):
    """Three members of the case's dims, the second and third moved by a few voxels in x and y: member 0 is the case's own
    volume (first and last pixel consumed), the others see the image off-centre."""
    shifts = [(0, 0, 0), (5, -2, 1), (-7, 3, -1)]
    return [capi.make_config(c.dims, c.vs, (c.origin + np.array(s, f32) * f32(c.vs)).astype(f32), K=c.K, im_height=c.hw[0],
                             im_width=c.hw[1], vol_id=i) for i, s in enumerate(shifts)]


# ------------------------------------------------------------------------------------------------------------------------
# oracle runs (the references of the GPU tests and the conditions of the CPU test)
# ------------------------------------------------------------------------------------------------------------------------
def integrate(oracle, cfg, depth, state=None, mask=None, c2b=EYE):
    """One frame into (t, w) (a fresh grid when None) by the oracle; returns the state."""
    dims = (cfg.dim_x, cfg.dim_y, cfg.dim_z)
    t, w = oracle.init_grid(dims) if state is None else state
    d = depth if mask is None else oracle.mask_depth(depth, mask)
    with np.errstate(invalid="ignore"):
        oracle.integrate(np.asarray(cfg.cam_K, f32), c2b, d, dims, np.asarray(cfg.origin, f32), cfg.voxel_size,
                         cfg.trunc_margin, t, w, max_depth=cfg.max_depth)
    return t, w


def integrate_colour(oracle, cfg, depth, rgb, state, colour=None, c2b=EYE):
    """The colour pass of a frame integrate() has just applied to `state`."""
    dims = (cfg.dim_x, cfg.dim_y, cfg.dim_z)
    colour = np.zeros(state[0].size, np.uint32) if colour is None else colour
    oracle.integrate_colour(np.asarray(cfg.cam_K, f32), c2b, depth, rgb, dims, np.asarray(cfg.origin, f32), cfg.voxel_size,
                            cfg.trunc_margin, state[1], colour, max_depth=cfg.max_depth)
    return colour


def integrate_labels(oracle, cfg, depth, label_im, score_im, labels=None, c2b=EYE, prob=0.5):
    dims = (cfg.dim_x, cfg.dim_y, cfg.dim_z)
    n = int(np.prod(dims))
    lab, fp, bp = labels if labels is not None else (np.zeros(n, np.uint16), np.zeros(n, f32), np.zeros(n, f32))
    oracle.integrate_labels(np.asarray(cfg.cam_K, f32), c2b, depth, label_im, score_im, dims, np.asarray(cfg.origin, f32),
                            cfg.voxel_size, cfg.trunc_margin, lab, fp, bp, max_depth=cfg.max_depth, prob_thd=prob)
    return lab, fp, bp


def differs(a, b):
    """Voxels (or elements) that differ in any bit between two tuples of arrays."""
    a = a if isinstance(a, tuple) else (a,)
    b = b if isinstance(b, tuple) else (b,)
    bad = np.zeros(a[0].size, bool)
    for x, y in zip(a, b):
        bad |= np.ascontiguousarray(x).view(np.uint8).reshape(x.size, -1).__ne__(
            np.ascontiguousarray(y).view(np.uint8).reshape(y.size, -1)).any(axis=1)
    return int(bad.sum())
