"""float32 NumPy restatement of the merge rule of csrc/tsdf_fuse.hip.h (tsdf_fuse_volume): every voxel of a destination
grid samples a source grid trilinearly at its own position and folds the sample in as one weighted observation.  Every
operation is float32 and in the order the kernel file states, so the device's TSDF, weights and counts equal these bit for
bit (a NaN result -- only possible where the destination already held a NaN, an infinity or a non-positive weight -- is
specified as "a NaN": compare with differs).  Test infrastructure; the product never imports it."""
import numpy as np

from semantic_slam_amd import capi

f32 = np.float32
COUNT_NAMES = ("sampled", "both", "both_band", "agree_band")


def relative_pose(base2world_src, base2world_dst):
    """M = inverse(base2world_src) * base2world_dst with the library's host helpers (a singular matrix: all-zero inverse)."""
    _, inv = capi.invert_matrix(np.asarray(base2world_src, f32))
    return capi.multiply_matrix(inv, np.asarray(base2world_dst, f32))


def pose_about(R, centre, shift=(0.0, 0.0, 0.0)):
    """Row-major 4x4 (16 float32) of the rigid motion that rotates by R about `centre` and then shifts."""
    R, c = np.asarray(R, np.float64), np.asarray(centre, np.float64)
    T = np.eye(4)
    T[:3, :3] = R
    T[:3, 3] = c - R @ c + np.asarray(shift, np.float64)
    return T.astype(f32).ravel()


def grid_of(cfg):
    """(dims, origin, voxel size, truncation, base2world) of a TsdfConfig, as the spec takes a grid."""
    return ((cfg.dim_x, cfg.dim_y, cfg.dim_z), np.asarray(cfg.origin, f32), f32(cfg.voxel_size), f32(cfg.trunc_margin),
            np.asarray(cfg.base2world, f32))


def fuse(dst_t, dst_w, dst_grid, src_t, src_w, src_grid, weight_thresh=0.9, agree_tol=0.4, write=1, info=None):
    """dst_* / src_*: flat float32 arrays, x fastest; *_grid: (dims, origin, vs, trunc, base2world).  Returns (tsdf, weight,
    counts) -- new arrays (the inputs are not changed; with write = 0 they are copies), counts a dict of COUNT_NAMES.
    info: a dict that receives "f" (the [n, 3] fractions f_i of the voxels inside the source box), the masks "inside" and
    "valid" (a valid sample the band test did not skip) over the destination, and how many valid voxels met each branch of the
    update: "fresh" (w_d == 0) and "observed"."""
    (ddx, ddy, ddz), od, vsd, trd, b2w_d = dst_grid
    (sdx, sdy, sdz), os_, vss, trs, b2w_s = src_grid
    od, os_ = np.asarray(od, f32), np.asarray(os_, f32)
    vsd, vss, thr, tol = f32(vsd), f32(vss), f32(weight_thresh), f32(agree_tol)
    M = relative_pose(b2w_s, b2w_d).reshape(4, 4)
    ratio = f32(trs) / f32(trd)
    dst_t = np.ascontiguousarray(dst_t, f32).ravel()
    dst_w = np.ascontiguousarray(dst_w, f32).ravel()
    src_t = np.ascontiguousarray(src_t, f32).ravel()
    src_w = np.ascontiguousarray(src_w, f32).ravel()
    n = ddx * ddy * ddz
    assert dst_t.size == n and dst_w.size == n and src_t.size == sdx * sdy * sdz and src_w.size == src_t.size
    with np.errstate(all="ignore"):
        # position
        x = [np.arange(d, dtype=np.int64).astype(f32) for d in (ddx, ddy, ddz)]
        p0 = (od[0] + x[0] * vsd)[None, None, :]
        p1 = (od[1] + x[1] * vsd)[None, :, None]
        p2 = (od[2] + x[2] * vsd)[:, None, None]
        g = []
        for i in range(3):
            q = ((M[i, 0] * p0 + M[i, 1] * p1) + M[i, 2] * p2) + M[i, 3]
            g.append(((q - os_[i]) / vss).astype(f32).ravel())
        hi = [f32(d - 1) for d in (sdx, sdy, sdz)]
        inside = np.ones(n, bool)
        for i in range(3):
            inside &= (g[i] >= f32(0)) & (g[i] <= hi[i])
        at = np.flatnonzero(inside)
        # sample
        gi = [g[i][at] for i in range(3)]
        j = [np.floor(a).astype(np.int64) for a in gi]
        f = [(a - b.astype(f32)).astype(f32) for a, b in zip(gi, j)]
        k = [np.where(fr > f32(0), b + 1, b) for fr, b in zip(f, j)]
        sy, sz = sdx, sdx * sdy
        corner = lambda a, b, c: (k[2] if c else j[2]) * sz + (k[1] if b else j[1]) * sy + (k[0] if a else j[0])
        order = [(0, 0, 0), (1, 0, 0), (0, 1, 0), (1, 1, 0), (0, 0, 1), (1, 0, 1), (0, 1, 1), (1, 1, 1)]
        idx = {c: corner(*c) for c in order}
        if at.size:
            assert min(int(v.min()) for v in idx.values()) >= 0 and max(int(v.max()) for v in idx.values()) < src_t.size
        c = {key: src_t[v] for key, v in idx.items()}
        w = {key: src_w[v] for key, v in idx.items()}
        wok = np.ones(at.size, bool)
        for key in order:
            wok &= w[key] > thr
        ws = w[order[0]].copy()
        for key in order[1:]:
            ws = np.where(w[key] < ws, w[key], ws)
        a = {(b, cc): c[(0, b, cc)] + f[0] * (c[(1, b, cc)] - c[(0, b, cc)]) for b in (0, 1) for cc in (0, 1)}
        b_ = {cc: a[(0, cc)] + f[1] * (a[(1, cc)] - a[(0, cc)]) for cc in (0, 1)}
        F = (b_[0] + f[2] * (b_[1] - b_[0])).astype(f32)
        valid = wok & np.isfinite(F)
        # band
        t = (F * ratio).astype(f32)
        valid &= ~(t <= f32(-1))
        t = np.where(t > f32(1), f32(1), t).astype(f32)
        # counts, with the destination's values before the update
        td, wd = dst_t[at], dst_w[at]
        both = valid & (wd > thr)
        band = both & (np.abs(td) < f32(1)) & (np.abs(t) < f32(1))
        agree = band & (np.abs(td - t) <= tol)
        counts = dict(zip(COUNT_NAMES, (int(valid.sum()), int(both.sum()), int(band.sum()), int(agree.sum()))))
        # update
        out_t, out_w = dst_t.copy(), dst_w.copy()
        if write:
            fresh = wd == f32(0)
            wn = (wd + ws).astype(f32)
            mean = ((td * wd + t * ws) / wn).astype(f32)
            new_t = np.where(fresh, t, mean).astype(f32)
            new_w = np.where(fresh, ws, wn).astype(f32)
            out_t[at[valid]] = new_t[valid]
            out_w[at[valid]] = new_w[valid]
    if info is not None:
        full_valid = np.zeros(n, bool)
        full_valid[at[valid]] = True
        info.update(f=np.stack(f, -1) if at.size else np.zeros((0, 3), f32), inside=inside, valid=full_valid,
                    fresh=int((valid & (wd == f32(0))).sum()), observed=int((valid & ~(wd == f32(0))).sum()))
    return out_t, out_w, counts


def differs(got, want):
    """Mask of the elements of got that differ from the spec's want: in any of the 32 bits where want is a number, in
    NaN-ness where it is a NaN."""
    got, want = np.ascontiguousarray(got, f32).ravel(), np.ascontiguousarray(want, f32).ravel()
    nan = np.isnan(want)
    return np.where(nan, ~np.isnan(got), got.view(np.uint32) != want.view(np.uint32))
