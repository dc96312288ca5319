"""Seeded random configurations shared by the randomised parity tests (test infrastructure): grid shapes of every shape
class, image sizes, intrinsics and volume placements (random_case), and TSDF / weight values drawn from the edges the
kernels' sign and weight tests meet (edge_values)."""
import numpy as np

f32 = np.float32
# thresholds the extraction entry points are called with: the default, the edges of the weight range, below every weight,
# and NaN (nothing passes `weight > NaN`)
THRESHOLDS = [0.0, 0.9, 1.0, 2.5, -1.0, float("nan")]
# a quiet NaN with a payload, so that a kernel that swapped it for the default NaN would show
NAN_PAYLOAD = np.array([0x7FC01234], np.uint32).view(f32)[0]
SPECIAL_T = np.array([NAN_PAYLOAD, np.inf, -np.inf, -0.0, 0.0, 1.0, -1.0], f32)


def random_case(seed):
    rng = np.random.default_rng(1000 + seed)
    shape_class = seed % 5
    if shape_class == 0:
        dims = (256 * int(rng.integers(1, 3)), int(rng.integers(3, 20)), int(rng.integers(2, 12)))   # row-mapped kernels
    elif shape_class == 1:
        dims = (4 * int(rng.integers(1, 90)), int(rng.integers(1, 40)), int(rng.integers(1, 20)))    # flat mapping
    elif shape_class == 2:
        dims = (int(rng.integers(1, 70)) | 1, int(rng.integers(1, 30)), int(rng.integers(1, 20)))    # odd rows: scalar kernel
    elif shape_class == 3:
        dims = (4, int(rng.integers(1, 5)), int(rng.integers(1, 5)))                                 # less than one chunk
    else:
        dims = (int(rng.integers(8, 40)) * 4, int(rng.integers(8, 40)), int(rng.integers(8, 30)))
    h, w = int(rng.integers(24, 200)), int(rng.integers(32, 260))
    K = np.array([rng.uniform(30, 400), 0, w / 2 + rng.uniform(-10, 10), 0, rng.uniform(30, 400),
                  h / 2 + rng.uniform(-10, 10), 0, 0, 1], np.float32)
    vs = float(rng.choice([0.003, 0.01, 0.02, 0.05]))
    ext = np.array(dims) * vs
    # volume placed so that cameras can end up inside, behind or beside it
    origin = (rng.uniform(-1.0, 0.2, 3) * ext + np.array([0, 0, rng.uniform(-0.5, 1.5)])).astype(np.float32)
    trunc = float(np.float32(vs) * np.float32(rng.choice([2, 5, 9])))
    max_depth = float(rng.choice([6.0, 2.5, 10.0]))
    return rng, dims, h, w, K, vs, origin, trunc, max_depth


def edge_values(rng, n, thr, p_special=0.25, p_weight=0.3):
    """TSDF and weight arrays of n voxels: ordinary values, and with the given odds the value edges -- NaN, +-inf, -0.0,
    0.0, +-1.0 as TSDF; the threshold itself, the next float above it, NaN, -1 and 0 as weight."""
    t = rng.uniform(-1.0, 1.0, n).astype(f32)
    pick = rng.uniform(0, 1, n) < p_special
    t[pick] = rng.choice(SPECIAL_T, int(pick.sum()))
    thr32 = f32(thr)
    base = thr32 if np.isfinite(thr32) else f32(0.9)
    w_edges = np.array([base, np.nextafter(base, f32(np.inf)), np.nan, -1.0, 0.0, 1.0, 2.0, 5.0], f32)
    w = rng.choice(np.array([1.0, 2.0, 3.0, 5.0], f32), n)
    pick = rng.uniform(0, 1, n) < p_weight
    w[pick] = rng.choice(w_edges, int(pick.sum()))
    return t, w
