"""float32 NumPy restatement of the carry rule of csrc/tsdf_fuse_carry.hip.h (tsdf_fuse_volume_carry), built on the merge's
restatement (fuse_spec.fuse and its info): the destination voxels a merge updates also take the source's colour, blended
with the merge's weights, and the source's label evidence as one observation.  Every operation is float32 in the order the
kernel file states; Fp / Bp are specified by their bits, a NaN as "a NaN" (fuse_spec.differs).  Test infrastructure; the
product never imports it."""
import numpy as np

import fuse_spec as fs

f32 = np.float32
COLOUR, LABELS = 1, 2
CARRY_COUNT_NAMES = ("label_adopted", "label_agreed", "label_opposed", "label_flipped")
ORDER = [(0, 0, 0), (1, 0, 0), (0, 1, 0), (1, 1, 0), (0, 0, 1), (1, 0, 1), (0, 1, 1), (1, 1, 1)]


def carried_cells(finfo, dst_grid, src_grid):
    """(flat destination indices of the carried voxels, j [3], f [3], k [3]) -- the positions re-derived with the merge's
    arithmetic and held to the fractions fuse_spec.fuse reports."""
    (ddx, ddy, ddz), od, vsd, _, b2w_d = dst_grid
    _, os_, vss, _, b2w_s = src_grid
    od, os_, vsd, vss = np.asarray(od, f32), np.asarray(os_, f32), f32(vsd), f32(vss)
    M = fs.relative_pose(b2w_s, b2w_d).reshape(4, 4)
    at = np.flatnonzero(finfo["valid"])
    x = [(at % ddx).astype(f32), ((at // ddx) % ddy).astype(f32), (at // (ddx * ddy)).astype(f32)]
    with np.errstate(all="ignore"):
        p = [od[i] + x[i] * vsd for i in range(3)]
        g = []
        for i in range(3):
            q = ((M[i, 0] * p[0] + M[i, 1] * p[1]) + M[i, 2] * p[2]) + M[i, 3]
            g.append(((q - os_[i]) / vss).astype(f32))
    j = [np.floor(a).astype(np.int64) for a in g]
    f = [(a - b.astype(f32)).astype(f32) for a, b in zip(g, j)]
    k = [np.where(fr > f32(0), b + 1, b) for fr, b in zip(f, j)]
    want_f = finfo["f"][finfo["valid"][np.flatnonzero(finfo["inside"])]]
    assert np.array_equal(np.stack(f, -1).view(np.uint32), want_f.view(np.uint32)) if at.size else True
    return at, j, f, k


def round_half_away(x):
    """roundf for the values that reach the conversion (0 <= r < 255): floor(x) + ((x - floor(x)) >= 0.5); the difference is
    exact in float32.  Elsewhere it lands on the same side of 0 and of 255 as roundf does (and is a NaN where x is)."""
    fl = np.floor(x).astype(f32)
    return (fl + ((x - fl) >= f32(0.5)).astype(f32)).astype(f32)


def fuse_carry(dst, dst_grid, src, src_grid, carry, prob_thd=0.5, weight_thresh=0.9, agree_tol=0.4, write=1, info=None):
    """dst / src: (tsdf, weight, colour uint32, label uint16, Fp, Bp), flat, x fastest; *_grid as fuse_spec.fuse takes them.
    Returns (the six destination arrays afterwards -- new arrays, the inputs are not changed --, counts): counts holds
    fuse_spec.COUNT_NAMES and CARRY_COUNT_NAMES.  info receives fuse_spec.fuse's entries and, over the carried voxels,
    "carried", "fresh" / "blended" (w_d == 0 or not), "adopted", "agreed", "flipped", "opposed_kept", "at_threshold" (opposed
    voxels whose Fp / (Fp + Bp) equals prob_thd: kept), "upper" (per axis, how
    many take the upper corner as nearest), "ties" (voxels with an f_i == 0.5), "half_up" (channels with x on a half that is
    rounded away from zero) and the channels that needed the clamp: "clamp_hi" (r > 255), "clamp_neg" (r < 0), "clamp_nan"."""
    dt, dw, dcol, dlab, dfp, dbp = dst
    st, sw, scol, slab, sfp, sbp = src
    assert carry in (0, 1, 2, 3)
    finfo = {}
    out_t, out_w, counts = fs.fuse(dt, dw, dst_grid, st, sw, src_grid, weight_thresh=weight_thresh, agree_tol=agree_tol,
                                   write=write, info=finfo)
    dw = np.ascontiguousarray(dw, f32).ravel()
    sw = np.ascontiguousarray(sw, f32).ravel()
    out_col = np.array(dcol, np.uint32).ravel()
    out_lab = np.array(dlab, np.uint16).ravel()
    out_fp, out_bp = np.array(dfp, f32).ravel(), np.array(dbp, f32).ravel()
    scol, slab = np.ascontiguousarray(scol, np.uint32).ravel(), np.ascontiguousarray(slab, np.uint16).ravel()
    sfp, sbp = np.ascontiguousarray(sfp, f32).ravel(), np.ascontiguousarray(sbp, f32).ravel()
    sdx, sdy, _ = src_grid[0]
    sy, sz = sdx, sdx * sdy
    at, j, f, k = carried_cells(finfo, dst_grid, src_grid)
    assert at.size == counts["sampled"]
    idx = {(a, b, c): (k[2] if c else j[2]) * sz + (k[1] if b else j[1]) * sy + (k[0] if a else j[0]) for a, b, c in ORDER}
    wd = dw[at]                                             # the weights BEFORE the merge
    stats = dict(carried=int(at.size), fresh=int((wd == f32(0)).sum()), blended=int((~(wd == f32(0))).sum()), half_up=0,
                 clamp_hi=0, clamp_neg=0, clamp_nan=0, upper=[int((fr >= f32(0.5)).sum()) for fr in f],
                 ties=int(((f[0] == f32(0.5)) | (f[1] == f32(0.5)) | (f[2] == f32(0.5))).sum()) if at.size else 0)
    with np.errstate(all="ignore"):
        if carry & COLOUR:
            ws = sw[idx[ORDER[0]]].copy()
            for key in ORDER[1:]:
                ws = np.where(sw[idx[key]] < ws, sw[idx[key]], ws)
            wn = (wd + ws).astype(f32)
            new = np.zeros(at.size, np.uint32)
            for s in (0, 8, 16):
                c = {key: ((scol[v] >> np.uint32(s)) & np.uint32(255)).astype(f32) for key, v in idx.items()}
                a = {(b, cc): c[(0, b, cc)] + f[0] * (c[(1, b, cc)] - c[(0, b, cc)]) for b in (0, 1) for cc in (0, 1)}
                b_ = {cc: a[(0, cc)] + f[1] * (a[(1, cc)] - a[(0, cc)]) for cc in (0, 1)}
                cs = (b_[0] + f[2] * (b_[1] - b_[0])).astype(f32)
                cd = ((out_col[at] >> np.uint32(s)) & np.uint32(255)).astype(f32)
                x = np.where(wd == f32(0), cs, ((cd * wd + cs * ws) / wn).astype(f32)).astype(f32)
                r = round_half_away(x)
                hi = r >= f32(255)
                ok = ~hi & (r >= f32(0))
                chan = np.where(hi, np.uint32(255), np.where(ok, r, f32(0)).astype(np.uint32)).astype(np.uint32)
                new |= chan << np.uint32(s)
                stats["clamp_hi"] += int((r > f32(255)).sum())
                stats["clamp_neg"] += int((r < f32(0)).sum())
                stats["clamp_nan"] += int(np.isnan(r).sum())
                stats["half_up"] += int((ok & ((x - np.floor(x)) == f32(0.5))).sum())
            if write:
                out_col[at] = new
        zero = dict.fromkeys(CARRY_COUNT_NAMES, 0)
        stats.update(adopted=0, agreed=0, flipped=0, opposed_kept=0, at_threshold=0)
        if carry & LABELS:
            n = [np.where(fr >= f32(0.5), b, a) for fr, a, b in zip(f, j, k)]
            near = n[2] * sz + n[1] * sy + n[0]
            Ls, Fs, Bs = slab[near], sfp[near], sbp[near]
            Ld, Fd, Bd = out_lab[at], out_fp[at], out_bp[at]
            act = Ls != 0
            adopted = act & (Ld == 0)
            agreed = act & (Ld != 0) & (Ld == Ls)
            opposed = act & (Ld != 0) & (Ld != Ls)
            b_opp = (Bd + Fs).astype(f32)
            ratio = (Fd / (Fd + b_opp)).astype(f32)
            flipped = opposed & (ratio < f32(prob_thd))
            stats["at_threshold"] = int((opposed & (ratio == f32(prob_thd))).sum())
            take = adopted | flipped
            new_l = np.where(take, Ls, Ld)
            new_f = np.where(take, Fs, np.where(agreed, (Fd + Fs).astype(f32), Fd))
            new_b = np.where(take, Bs, np.where(agreed, (Bd + Bs).astype(f32), np.where(opposed, b_opp, Bd)))
            if write:
                out_lab[at], out_fp[at], out_bp[at] = new_l, new_f, new_b
            zero = dict(zip(CARRY_COUNT_NAMES, (int(adopted.sum()), int(agreed.sum()), int(opposed.sum()), int(flipped.sum()))))
            stats.update(adopted=int(adopted.sum()), agreed=int(agreed.sum()), flipped=int(flipped.sum()),
                         opposed_kept=int((opposed & ~flipped).sum()))
    counts = dict(counts, **zero)
    if info is not None:
        info.update(finfo)
        info.update(stats)
    return (out_t, out_w, out_col, out_lab, out_fp, out_bp), counts
