"""The extent rule (semantic_slam_amd/csrc/tsdf_extent.hip.h) restated in NumPy with exact Python integers (test
infrastructure): classification in float32, every sum as a Python int, so the record is specified bit for bit.  Also the
host-only calls' arithmetic -- combine, metric (double), regrid (float32 origin) -- as the header states it.

A record is a dict of Python ints and lists of ints, the shape of capi.Extent.as_dict():
    n_observed, n_surface, sum [3] (x, y, z), sum2 [6] (xx, yy, zz, xy, xz, yz), border [6] (x-, x+, y-, y+, z-, z+),
    lo [3], hi [3]
"""
import numpy as np

f32 = np.float32
PAIRS = ((0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2))     # the order of sum2 and of the covariance


def classify(t, w, weight_thresh=0.9, band=1.0):
    """(observed, surface) per voxel: observed = w > weight_thresh; surface = observed && fabsf(t) < band, in float32
    (a comparison with a NaN is false)."""
    t, w = np.asarray(t, f32), np.asarray(w, f32)
    with np.errstate(invalid="ignore"):
        observed = w > f32(weight_thresh)
        surface = observed & (np.abs(t) < f32(band))
    return observed, surface


def extent(t, w, dims, z_begin=0, z_end=None, weight_thresh=0.9, band=1.0, margin=0):
    """The record of the slab [z_begin, z_end) of a grid of GLOBAL dims (x, y, z); t, w hold the slab's voxels, x fastest.
    Indices, bounds and the z faces are in global z."""
    dx, dy, dz = (int(d) for d in dims)
    z_end = dz if z_end is None else int(z_end)
    nz = z_end - z_begin
    observed, surface = classify(t, w, weight_thresh, band)
    assert observed.size == dx * dy * nz
    zi, yi, xi = np.nonzero(surface.reshape(nz, dy, dx))
    n = len(xi)
    if n * max(dx, dy, dz) ** 2 < 2 ** 62:
        # no sum can leave int64: NumPy's integer sums are exact and the record is made of Python ints all the same
        idx = [xi.astype(np.int64), yi.astype(np.int64), zi.astype(np.int64) + z_begin]
        total = lambda a: int(a.sum(dtype=np.int64))
        count = lambda hit: int(np.count_nonzero(hit))
        product = lambda p, q: p * q
    else:
        idx = [[int(v) for v in xi], [int(v) for v in yi], [int(v) + z_begin for v in zi]]     # Python ints from here on
        total, count = sum, sum
        product = lambda p, q: [a * b for a, b in zip(p, q)]
        idx = [_Ints(a) for a in idx]
    rec = {"n_observed": int(observed.sum()), "n_surface": n,
           "sum": [total(a) for a in idx],
           "sum2": [total(product(idx[i], idx[j])) for i, j in PAIRS],
           "border": [], "lo": [dx, dy, dz], "hi": [-1, -1, -1]}
    for axis, d in enumerate((dx, dy, dz)):
        rec["border"].append(count(idx[axis] < margin))
        rec["border"].append(count(idx[axis] >= d - margin))
        if n:
            rec["lo"][axis], rec["hi"][axis] = int(min(idx[axis])), int(max(idx[axis]))
    return rec


class _Ints(list):
    """A list of Python ints that compares element by element, as the arrays of the int64 path do."""

    def __lt__(self, bound):
        return [v < bound for v in self]

    def __ge__(self, bound):
        return [v >= bound for v in self]


def empty(dims):
    return {"n_observed": 0, "n_surface": 0, "sum": [0] * 3, "sum2": [0] * 6, "border": [0] * 6,
            "lo": [int(d) for d in dims], "hi": [-1] * 3}


def combine(a, b):
    """Two disjoint sets of voxels of one grid: sums added (modulo 2^64, as the C struct holds them), bounds by min / max."""
    m = (1 << 64) - 1
    out = {"n_observed": (a["n_observed"] + b["n_observed"]) & m, "n_surface": (a["n_surface"] + b["n_surface"]) & m}
    for k in ("sum", "sum2", "border"):
        out[k] = [(p + q) & m for p, q in zip(a[k], b[k])]
    out["lo"] = [min(p, q) for p, q in zip(a["lo"], b["lo"])]
    out["hi"] = [max(p, q) for p, q in zip(a["hi"], b["hi"])]
    return out


def metric(rec, origin, voxel_size, base2world):
    """Double arithmetic in the header's order: mean = sum / n; centroid_base = origin + mean * vs; centroid_world through
    base2world (row-major 4x4); cov = (sum2 / n - mean_i * mean_j) * (vs * vs); lo_base / hi_base the outer corners."""
    n, vs = float(rec["n_surface"]), float(f32(voxel_size))
    o = [float(f32(v)) for v in origin]
    B = [float(f32(v)) for v in np.asarray(base2world).ravel()]
    mean = [float(s) / n for s in rec["sum"]]
    cb = [o[i] + mean[i] * vs for i in range(3)]
    cw = [((B[4 * i] * cb[0] + B[4 * i + 1] * cb[1]) + B[4 * i + 2] * cb[2]) + B[4 * i + 3] for i in range(3)]
    cov = [(float(rec["sum2"][k]) / n - mean[i] * mean[j]) * (vs * vs) for k, (i, j) in enumerate(PAIRS)]
    return {"centroid_base": np.array(cb), "centroid_world": np.array(cw), "cov_base": np.array(cov),
            "lo_base": np.array([o[i] + (float(rec["lo"][i]) - 0.5) * vs for i in range(3)]),
            "hi_base": np.array([o[i] + (float(rec["hi"][i]) + 0.5) * vs for i in range(3)])}


def regrid(rec, origin, voxel_size, pad_voxels, dim_multiple):
    """(dims, origin float32 [3]) of the proposed grid: origin_i + (float)(lo_i - pad) * vs as two rounded float32
    operations; hi - lo + 1 + 2 pad rounded up to a multiple."""
    dims, out = [], np.empty(3, f32)
    for i in range(3):
        d = rec["hi"][i] - rec["lo"][i] + 1 + 2 * pad_voxels
        dims.append((d + dim_multiple - 1) // dim_multiple * dim_multiple)
        out[i] = f32(origin[i]) + f32(f32(rec["lo"][i] - pad_voxels) * f32(voxel_size))
    return tuple(dims), out
