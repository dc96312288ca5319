"""Float32 NumPy restatement of the registration rule of csrc/tsdf_align.hip.h (the header comment states it; this follows it
line by line).  Per-voxel values are np.float32 evaluated in the header's order, so every pair decision and every per-pair term
is the device's bit for bit; the sums and the solve are float64 and are tests/track_spec.py's (the rule says "exactly
tsdf_track's").  The parity contract is track_spec's: the system of a single pair equals the double value of these float32
terms; a system of n pairs is within n * 2^-52 * sum |term| per entry with the pair count exact; a run's status, iters_run and
pairs are equal, its rmse and every entry of its float32 pose within one float32 ulp.  Test infrastructure; the product never
imports it.

    params(...)                                      the dict of tsdf_align_params' fields (from_ctypes: of a capi.AlignParams)
    start_pose(grids, guess=None)                    M [3, 4] float64: the guess's float32 entries, or fuse_spec.relative_pose
    pair_terms(dst, src, grids, Rm, tm, level, P)    per-pair terms [n, 29] float32 (info: rejects per gate, near misses, idx)
    system(dst, src, grids, M, level, P)             (sums [29] float64, sum |term| [29] float64)
    align(dst, src, grids, P, guess=None)            dict M, dst2src, status, iters_run, pairs, rmse, lost (history: per iteration)
    fuse_at(..., dst2src)                            fuse_spec.fuse with M replaced by the given float32 entries

dst = (tsdf, weight), src = (tsdf, weight): flat float32 arrays, x fastest; grids = (dst grid, src grid), each
(dims, origin, vs, trunc, base2world) as fuse_spec.grid_of gives it.
"""
import math

import numpy as np

import fuse_spec as fs
import track_spec as ts

f32 = np.float32
N_TERMS = ts.N_TERMS
UPPER = ts.UPPER
# every lattice point is counted at the first gate that turns it away, in the rule's order
GATES = ("candidate", "box", "corner", "finite", "band", "resid", "normal")


def params(weight_thresh=0.9, resid_thresh=1.0, n_levels=2, iters=(10, 10, 0), min_pairs=300, eps_rot=1e-5, eps_trans=1e-5):
    return {"weight_thresh": f32(weight_thresh), "resid_thresh": f32(resid_thresh), "n_levels": int(n_levels),
            "iters": list(iters), "min_pairs": int(min_pairs), "eps_rot": float(f32(eps_rot)), "eps_trans": float(f32(eps_trans))}


def from_ctypes(p):
    """The dict of a capi.AlignParams."""
    return params(p.weight_thresh, p.resid_thresh, p.n_levels, list(p.iters), p.min_pairs, p.eps_rot, p.eps_trans)


def pose_default(grids):
    """float32 [16]: the matrix tsdf_fuse_volume composes (tsdf_fuse_pose_default)."""
    return np.asarray(fs.relative_pose(grids[1][4], grids[0][4]), f32).ravel()


def start_pose(grids, guess=None):
    m = pose_default(grids) if guess is None else np.asarray(guess, f32).ravel()
    return m.astype(np.float64).reshape(4, 4)[:3].copy()


def lattice(dims, level):
    """(x, y, z) int64 voxel indices of the level's lattice, x fastest, and (points per axis, stride)."""
    s = 1 << level
    ln = [-(-d // s) for d in dims]
    lz, ly, lx = np.meshgrid(np.arange(ln[2]), np.arange(ln[1]), np.arange(ln[0]), indexing="ij")
    return (s * lx.ravel(), s * ly.ravel(), s * lz.ravel()), ln, s


def _spacing(a):
    return np.spacing(np.abs(np.asarray(a, f32)))


def pair_terms(dst, src, grids, Rm, tm, level, P, info=None):
    """terms [n_pairs, 29] float32 in lattice order.  info, a dict, receives "lattice" (its size), "candidates", "rejected" (a
    dict of GATES), "idx" (the flat lattice index (lz * ln_y + ly) * ln_x + lx of every pair), "near" (a dict: per computed
    comparison -- box, band, resid, normal -- how many values lie within one float32 spacing of their threshold without
    being equal to it; equality comes from exact inputs, such as eight free-space corners of 1.0, and is decided alike by
    any IEEE arithmetic), and "pairs_q" (the q of the pairs, [n, 3])."""
    (ddims, od, vsd, trd, _), (sdims, os_, vss, trs, _) = grids
    od, os_ = np.asarray(od, f32), np.asarray(os_, f32)
    vsd, vss = f32(vsd), f32(vss)
    thr, rthr = f32(P["weight_thresh"]), f32(P["resid_thresh"])
    dt = np.ascontiguousarray(dst[0], f32).ravel()
    dw = np.ascontiguousarray(dst[1], f32).ravel()
    st = np.ascontiguousarray(src[0], f32).ravel()
    sw = np.ascontiguousarray(src[1], f32).ravel()
    assert dt.size == int(np.prod(ddims)) == dw.size and st.size == int(np.prod(sdims)) == sw.size and min(sdims) >= 2
    Rm = np.asarray(Rm, f32).reshape(3, 3)
    tm = np.asarray(tm, f32).ravel()
    (x0, x1, x2), ln, s = lattice(ddims, level)
    flat = np.arange(x0.size)
    left = [x0.size]
    near = {}
    with np.errstate(all="ignore"):
        at = (x2 * ddims[1] + x1) * ddims[0] + x0
        td, wd = dt[at], dw[at]
        keep = (wd > thr) & (np.abs(td) < f32(1))
        x0, x1, x2, td, flat = x0[keep], x1[keep], x2[keep], td[keep], flat[keep]
        left.append(x0.size)
        p = [od[0] + x0.astype(f32) * vsd, od[1] + x1.astype(f32) * vsd, od[2] + x2.astype(f32) * vsd]
        q = [((Rm[i, 0] * p[0] + Rm[i, 1] * p[1]) + Rm[i, 2] * p[2]) + tm[i] for i in range(3)]
        g = [((q[i] - os_[i]) / vss).astype(f32) for i in range(3)]
        hi = [f32(d - 1) for d in sdims]
        keep = np.ones(x0.size, bool)
        nb = 0
        for i in range(3):
            keep &= (g[i] >= f32(0)) & (g[i] < hi[i])
            nb += int(((g[i] != 0) & (np.abs(g[i]) <= _spacing(g[i]))).sum())
            nb += int(((g[i] != hi[i]) & (np.abs(g[i] - hi[i]) <= np.maximum(_spacing(g[i]), _spacing(hi[i])))).sum())
        near["box"] = nb
        td, flat = td[keep], flat[keep]
        q, g = [a[keep] for a in q], [a[keep] for a in g]
        left.append(td.size)
        j = [np.floor(a).astype(np.int64) for a in g]
        f = [(a - b.astype(f32)).astype(f32) for a, b in zip(g, j)]
        sy, sz = sdims[0], sdims[0] * sdims[1]
        base = j[2] * sz + j[1] * sy + j[0]
        if base.size:
            assert int(base.min()) >= 0 and int(base.max()) + sz + sy + 1 < st.size
        idx = {(a, b, c): base + c * sz + b * sy + a for a in (0, 1) for b in (0, 1) for c in (0, 1)}
        wok = np.ones(td.size, bool)
        for key in idx:
            wok &= sw[idx[key]] > thr
        c = {key: st[v] for key, v in idx.items()}
        d = {(b, cc): c[(1, b, cc)] - c[(0, b, cc)] for b in (0, 1) for cc in (0, 1)}
        a_ = {(b, cc): c[(0, b, cc)] + f[0] * d[(b, cc)] for b in (0, 1) for cc in (0, 1)}
        h = {cc: a_[(1, cc)] - a_[(0, cc)] for cc in (0, 1)}
        b_ = {cc: a_[(0, cc)] + f[1] * h[cc] for cc in (0, 1)}
        G2 = b_[1] - b_[0]
        F = b_[0] + f[2] * G2
        e = {cc: d[(0, cc)] + f[1] * (d[(1, cc)] - d[(0, cc)]) for cc in (0, 1)}
        G0 = e[0] + f[2] * (e[1] - e[0])
        G1 = h[0] + f[2] * (h[1] - h[0])
        ratio = f32(trs) / f32(trd)
        gscale = ratio / vss
        t = (F * ratio).astype(f32)
        r = (t - td).astype(f32)
        n = [(G * gscale).astype(f32) for G in (G0, G1, G2)]
        keep = wok
        left.append(int(keep.sum()))
        keep = keep & np.isfinite(F)
        left.append(int(keep.sum()))
        live = keep.copy()                      # the near misses are looked for among the points still alive at each gate
        at1 = np.abs(t)
        near["band"] = int((live & (at1 != 1) & (np.abs(at1 - f32(1)) <= np.maximum(_spacing(at1), _spacing(f32(1))))).sum())
        keep = keep & (np.abs(t) < f32(1))
        left.append(int(keep.sum()))
        ar = np.abs(r)
        near["resid"] = int((keep & (ar != rthr) & (np.abs(ar - rthr) <= np.maximum(_spacing(ar), _spacing(rthr)))).sum())
        keep = keep & (np.abs(r) <= rthr)
        left.append(int(keep.sum()))
        nn = (n[0] * n[0] + n[1] * n[1]) + n[2] * n[2]
        near["normal"] = int((keep & (nn != 0) & (np.abs(nn) <= _spacing(nn))).sum())
        keep = keep & np.isfinite(n[0]) & np.isfinite(n[1]) & np.isfinite(n[2]) & (nn > f32(0))
        left.append(int(keep.sum()))
        sel = lambda v: v[keep]
        q, n, r = [sel(v) for v in q], [sel(v) for v in n], sel(r)
        J = [q[1] * n[2] - q[2] * n[1], q[2] * n[0] - q[0] * n[2], q[0] * n[1] - q[1] * n[0], n[0], n[1], n[2]]
        cols = [J[a] * J[b] for a, b in UPPER] + [J[a] * r for a in range(6)] + [r * r, np.ones_like(r)]
    if info is not None:
        info["lattice"] = left[0]
        info["candidates"] = left[1]
        info["rejected"] = {gate: left[k] - left[k + 1] for k, gate in enumerate(GATES)}
        info["idx"] = flat[keep]
        info["near"] = near
        info["pairs_q"] = np.stack(q, -1) if r.size else np.zeros((0, 3), f32)
    return np.stack(cols, axis=1).astype(f32)


def system(dst, src, grids, M, level, P, info=None):
    M = np.asarray(M, np.float64).reshape(-1)[:12].reshape(3, 4)
    t64 = pair_terms(dst, src, grids, M[:, :3].astype(f32), M[:, 3].astype(f32), level, P, info).astype(np.float64)
    return t64.sum(axis=0), np.abs(t64).sum(axis=0)


def result_pose(M):
    out = np.zeros((4, 4), f32)
    out[:3] = np.asarray(M, np.float64).astype(f32)
    out[3, 3] = 1
    return out.ravel()


def align(dst, src, grids, P, guess=None, history=None):
    """history, a list, receives one dict per iteration that ran: level, pairs, w and tau (|w|, |tau| of the step; None when
    there was none), pivot_ratio (track_spec.cholesky_solve's; None when min_pairs decided), lost, done, near (pair_terms')."""
    M = start_pose(grids, guess)
    start = pose_default(grids) if guess is None else np.asarray(guess, f32).ravel().copy()
    lost, done, iters_run, pairs, r2 = False, [0, 0, 0], [0, 0, 0], 0, 0.0
    for lvl in range(P["n_levels"] - 1, -1, -1):
        for _ in range(P["iters"][lvl]):
            if lost or done[lvl]:
                break
            info = {}
            sys, _ = system(dst, src, grids, M, lvl, P, info)
            pairs, r2 = int(sys[28]), float(sys[27])
            iters_run[lvl] += 1
            note = {"level": lvl, "pairs": pairs, "w": None, "tau": None, "pivot_ratio": None, "lost": False, "done": False,
                    "near": info["near"], "lattice": info["lattice"]}
            if history is not None:
                history.append(note)
            xi = ts.cholesky_solve(sys, note) if sys[28] >= P["min_pairs"] else None
            if xi is None:
                lost = note["lost"] = True
                break
            M = ts.step(M, xi)
            th = math.sqrt((xi[0] * xi[0] + xi[1] * xi[1]) + xi[2] * xi[2])
            tn = math.sqrt((xi[3] * xi[3] + xi[4] * xi[4]) + xi[5] * xi[5])
            note["w"], note["tau"] = th, tn
            if th < P["eps_rot"] and tn < P["eps_trans"]:
                done[lvl] = 1
                note["done"] = True
    ran = [lvl for lvl in range(P["n_levels"]) if P["iters"][lvl] > 0]
    status = 2 if lost else (0 if ran and done[ran[0]] else 1)
    pose = result_pose(M)
    if lost:                                   # the starting matrix's own bits, all 16
        pose = start
    return {"M": M, "dst2src": pose, "status": status, "iters_run": iters_run, "pairs": pairs, "lost": lost,
            "rmse": math.sqrt(r2 / pairs) if pairs > 0 else 0.0}


def fuse_at(dst_t, dst_w, dst_grid, src_t, src_w, src_grid, dst2src, **kw):
    """fuse_spec.fuse with M replaced by the float32 entries of dst2src and nothing else of the rule changed (fuse looks
    relative_pose up in its module; it is put back afterwards)."""
    m = np.asarray(dst2src, f32).ravel().copy()
    assert m.size == 16
    saved = fs.relative_pose
    fs.relative_pose = lambda b2w_src, b2w_dst: m
    try:
        return fs.fuse(dst_t, dst_w, dst_grid, src_t, src_w, src_grid, **kw)
    finally:
        fs.relative_pose = saved


def motion_error(dst2src, truth, centre=(0.0, 0.0, 0.0)):
    """(rotation error in degrees, translation error in metres) of a dst2src against the true one; the translation error is
    the distance between the two images of `centre` (destination base coordinates: the scene's centre, so that the lever
    arm of the rotation error about a far-away origin does not count as translation)."""
    A, B = np.asarray(dst2src, np.float64).reshape(4, 4), np.asarray(truth, np.float64).reshape(4, 4)
    _, e_r = ts.pose_error(A, B)
    c = np.append(np.asarray(centre, np.float64), 1.0)
    return math.degrees(e_r), float(np.linalg.norm((A @ c - B @ c)[:3]))
