"""Float32 NumPy restatement of the scan tracking rule of csrc/tsdf_scan_track.hip.h (the header comment states it; this follows
it line by line).  Per-point values are np.float32 evaluated in the header's order, so every pair decision and every per-pair
term is the device's bit for bit; the sums and the solve are float64 and are tests/track_spec.py's (the rule says "exactly
tsdf_track's").  The parity contract is track_spec's and align_spec's: the system of a single pair equals the double value of
these float32 terms; a system of n pairs is within n * 2^-52 * sum |term| per entry with the pair count exact; a run's status,
iters_run and pairs are equal, its rmse and every entry of its float32 pose within one float32 ulp.  Test infrastructure; the
product never imports it.

    params(trunc, ...)                                  the dict of tsdf_scan_track_params' fields (from_ctypes: of a capi.ScanTrackParams)
    scan_pose(R_rect, R_velo, t_velo)                   tsdf_scan_pose: velo2cam float32 [16]
    start_pose(grid, velo2world)                        M [3, 4] float64: the rule's "Pose"
    pair_terms(vol, grid, points, flags, Rm, tm, level, P)    per-pair terms [n, 29] float32 (info: rejects per gate, near misses, idx)
    pair_terms_scalar(...)                              the same, one point at a time in np.float32 scalars
    system(vol, grid, points, flags, M, level, P)       (sums [29] float64, sum |term| [29] float64)
    track(vol, grid, points, flags, P, guess)           dict M, velo2world, status, iters_run, pairs, rmse, lost

vol = (tsdf, weight): flat float32 arrays, x fastest; grid = (dims, origin, vs, trunc, base2world) as fuse_spec.grid_of gives
it; points: [n, 4] float32; flags: [n] uint8 or None.
"""
import math

import numpy as np

import track_spec as ts
from semantic_slam_amd import capi

f32 = np.float32
N_TERMS = ts.N_TERMS
UPPER = ts.UPPER
# every selected point is counted at the first gate that turns it away, in the rule's order
GATES = ("finite", "range", "flag", "box", "corner", "value", "band", "resid", "normal")


def params(trunc, weight_thresh=0.9, resid_thresh=None, min_range_m=2.5, max_range_m=80.0, n_levels=3, iters=(10, 5, 4),
           min_pairs=300, drop_flag=-1, eps_rot=1e-5, eps_trans=1e-5):
    return {"weight_thresh": f32(weight_thresh), "resid_thresh": f32(trunc if resid_thresh is None else resid_thresh),
            "min_range_m": f32(min_range_m), "max_range_m": f32(max_range_m), "n_levels": int(n_levels), "iters": list(iters),
            "min_pairs": int(min_pairs), "drop_flag": int(drop_flag), "eps_rot": float(f32(eps_rot)),
            "eps_trans": float(f32(eps_trans))}


def from_ctypes(p):
    """The dict of a capi.ScanTrackParams."""
    return params(None, p.weight_thresh, p.resid_thresh, p.min_range_m, p.max_range_m, p.n_levels, list(p.iters), p.min_pairs,
                  p.drop_flag, p.eps_rot, p.eps_trans)


def to_ctypes(P):
    """The capi.ScanTrackParams of a spec dict."""
    p = capi.ScanTrackParams()
    p.weight_thresh, p.resid_thresh = float(P["weight_thresh"]), float(P["resid_thresh"])
    p.min_range_m, p.max_range_m, p.n_levels = float(P["min_range_m"]), float(P["max_range_m"]), P["n_levels"]
    p.iters[:] = list(P["iters"])
    p.min_pairs, p.drop_flag, p.eps_rot, p.eps_trans = P["min_pairs"], P["drop_flag"], P["eps_rot"], P["eps_trans"]
    return p


def _mul4_f32(a, b):
    """tsdf_multiply_matrix's order: each entry a left-to-right float32 sum over k."""
    a, b = np.asarray(a, f32).reshape(4, 4), np.asarray(b, f32).reshape(4, 4)
    out = np.zeros((4, 4), f32)
    with np.errstate(all="ignore"):
        for i in range(4):
            for j in range(4):
                acc = f32(a[i, 0] * b[0, j])
                for k in range(1, 4):
                    acc = f32(acc + f32(a[i, k] * b[k, j]))
                out[i, j] = acc
    return out


def scan_pose(R_rect, R_velo, t_velo):
    A, B = np.zeros((4, 4), f32), np.zeros((4, 4), f32)
    A[:3, :3] = np.asarray(R_rect, f32).reshape(3, 3)
    B[:3, :3] = np.asarray(R_velo, f32).reshape(3, 3)
    B[:3, 3] = np.asarray(t_velo, f32).ravel()
    A[3, 3] = B[3, 3] = 1
    return _mul4_f32(A, B).ravel()


def start_pose(grid, velo2world):
    """float32 multiply_matrix(base2world_inv, [the first three rows of velo2world; 0 0 0 1]), its first three rows in double."""
    g = np.zeros(16, f32)
    g[:12] = np.asarray(velo2world, f32).ravel()[:12]
    g[15] = 1
    _, inv = capi.invert_matrix(np.asarray(grid[4], f32))
    return _mul4_f32(inv, g).astype(np.float64)[:3].copy()


def selected(n_points, level):
    """The indices of the level's points, in scan order."""
    return np.arange(0, n_points, 1 << level, dtype=np.int64)


def _spacing(a):
    return np.spacing(np.abs(np.asarray(a, f32)))


def _near(v, thr):
    """How many of v lie within one float32 spacing of thr without being equal to it."""
    v = np.asarray(v, f32)
    with np.errstate(all="ignore"):
        return int(((v != thr) & (np.abs(v - thr) <= np.maximum(_spacing(v), _spacing(thr)))).sum())


def pair_terms(vol, grid, points, flags, Rm, tm, level, P, info=None):
    """terms [n_pairs, 29] float32 in scan order.  info, a dict, receives "selected" (the level's points), "rejected" (a dict of
    GATES), "idx" (the point index of every pair), "near" (a dict: per computed comparison -- range, box, band, resid, normal --
    how many values lie within one float32 spacing of their threshold without being equal to it) and "pairs_q"."""
    dims, org, vs, trunc, _ = grid
    org, vs, tr = np.asarray(org, f32), f32(vs), f32(trunc)
    thr, rthr = f32(P["weight_thresh"]), f32(P["resid_thresh"])
    t = np.ascontiguousarray(vol[0], f32).ravel()
    w = np.ascontiguousarray(vol[1], f32).ravel()
    assert t.size == int(np.prod(dims)) == w.size and min(dims) >= 2
    pts = np.ascontiguousarray(points, f32).reshape(-1, 4)
    Rm = np.asarray(Rm, f32).reshape(3, 3)
    tm = np.asarray(tm, f32).ravel()
    at = selected(len(pts), level)
    left = [at.size]
    near = {}
    with np.errstate(all="ignore"):
        x, y, z = pts[at, 0], pts[at, 1], pts[at, 2]
        keep = np.isfinite(x) & np.isfinite(y) & np.isfinite(z)
        left.append(int(keep.sum()))
        d2 = (x * x + y * y) + z * z
        rmin2, rmax2 = f32(P["min_range_m"] * P["min_range_m"]), f32(P["max_range_m"] * P["max_range_m"])
        near["range"] = _near(d2[keep], rmin2) + _near(d2[keep], rmax2)
        keep &= (d2 >= rmin2) & (d2 <= rmax2)
        left.append(int(keep.sum()))
        if flags is not None and P["drop_flag"] >= 0:
            keep &= np.asarray(flags, np.uint8).ravel()[at].astype(np.int64) != P["drop_flag"]
        left.append(int(keep.sum()))
        at, x, y, z = at[keep], x[keep], y[keep], z[keep]
        q = [((Rm[i, 0] * x + Rm[i, 1] * y) + Rm[i, 2] * z) + tm[i] for i in range(3)]
        g = [((q[i] - org[i]) / vs).astype(f32) for i in range(3)]
        hi = [f32(d - 1) for d in dims]
        keep = np.ones(at.size, bool)
        near["box"] = 0
        for i in range(3):
            keep &= (g[i] >= f32(0)) & (g[i] < hi[i])
            near["box"] += _near(g[i], f32(0)) + _near(g[i], hi[i])
        at = at[keep]
        q, g = [a[keep] for a in q], [a[keep] for a in g]
        left.append(at.size)
        j = [np.floor(a).astype(np.int64) for a in g]
        f = [(a - b.astype(f32)).astype(f32) for a, b in zip(g, j)]
        sy, sz = dims[0], dims[0] * dims[1]
        base = j[2] * sz + j[1] * sy + j[0]
        if base.size:
            assert int(base.min()) >= 0 and int(base.max()) + sz + sy + 1 < t.size
        idx = {(a, b, c): base + c * sz + b * sy + a for a in (0, 1) for b in (0, 1) for c in (0, 1)}
        wok = np.ones(at.size, bool)
        for key in idx:
            wok &= w[idx[key]] > thr
        c = {key: t[v] for key, v in idx.items()}
        d = {(b, cc): c[(1, b, cc)] - c[(0, b, cc)] for b in (0, 1) for cc in (0, 1)}
        a_ = {(b, cc): c[(0, b, cc)] + f[0] * d[(b, cc)] for b in (0, 1) for cc in (0, 1)}
        h = {cc: a_[(1, cc)] - a_[(0, cc)] for cc in (0, 1)}
        b_ = {cc: a_[(0, cc)] + f[1] * h[cc] for cc in (0, 1)}
        G2 = b_[1] - b_[0]
        F = b_[0] + f[2] * G2
        e = {cc: d[(0, cc)] + f[1] * (d[(1, cc)] - d[(0, cc)]) for cc in (0, 1)}
        G0 = e[0] + f[2] * (e[1] - e[0])
        G1 = h[0] + f[2] * (h[1] - h[0])
        gscale = tr / vs
        r = (F * tr).astype(f32)
        n = [(G * gscale).astype(f32) for G in (G0, G1, G2)]
        keep = wok
        left.append(int(keep.sum()))
        keep = keep & np.isfinite(F)
        left.append(int(keep.sum()))
        aF = np.abs(F)
        near["band"] = _near(aF[keep], f32(1))
        keep = keep & (aF < f32(1))
        left.append(int(keep.sum()))
        ar = np.abs(r)
        near["resid"] = _near(ar[keep], rthr)
        keep = keep & (ar <= rthr)
        left.append(int(keep.sum()))
        nn = (n[0] * n[0] + n[1] * n[1]) + n[2] * n[2]
        near["normal"] = _near(nn[keep], f32(0))
        keep = keep & np.isfinite(n[0]) & np.isfinite(n[1]) & np.isfinite(n[2]) & (nn > f32(0))
        left.append(int(keep.sum()))
        sel = lambda v: v[keep]
        q, n, r = [sel(v) for v in q], [sel(v) for v in n], sel(r)
        J = [q[1] * n[2] - q[2] * n[1], q[2] * n[0] - q[0] * n[2], q[0] * n[1] - q[1] * n[0], n[0], n[1], n[2]]
        cols = [J[a] * J[b] for a, b in UPPER] + [J[a] * r for a in range(6)] + [r * r, np.ones_like(r)]
    if info is not None:
        info["selected"] = left[0]
        info["rejected"] = {gate: left[k] - left[k + 1] for k, gate in enumerate(GATES)}
        info["idx"] = at[keep]
        info["near"] = near
        info["pairs_q"] = np.stack(q, -1) if r.size else np.zeros((0, 3), f32)
    return np.stack(cols, axis=1).astype(f32).reshape(-1, N_TERMS)


def pair_terms_scalar(vol, grid, points, flags, Rm, tm, level, P, info=None):
    """The second statement of the per-point rule: one point at a time, every value an np.float32 scalar, the header's gates
    as a chain of early returns.  info receives "idx" and "rejected" as pair_terms gives them."""
    dims, org, vs, trunc, _ = grid
    org, vs, tr = [f32(o) for o in org], f32(vs), f32(trunc)
    thr, rthr = f32(P["weight_thresh"]), f32(P["resid_thresh"])
    with np.errstate(over="ignore"):
        rmin2, rmax2 = f32(P["min_range_m"] * P["min_range_m"]), f32(P["max_range_m"] * P["max_range_m"])
    gscale = f32(tr / vs)
    t = np.ascontiguousarray(vol[0], f32).ravel()
    w = np.ascontiguousarray(vol[1], f32).ravel()
    pts = np.ascontiguousarray(points, f32).reshape(-1, 4)
    Rm = np.asarray(Rm, f32).reshape(3, 3)
    tm = np.asarray(tm, f32).ravel()
    hi = [f32(d - 1) for d in dims]
    sy, sz = dims[0], dims[0] * dims[1]
    one, zero = f32(1), f32(0)
    rejected = dict.fromkeys(GATES, 0)
    rows, idx = [], []

    def one_point(k):
        x, y, z = pts[k, 0], pts[k, 1], pts[k, 2]
        if not (np.isfinite(x) and np.isfinite(y) and np.isfinite(z)):
            return "finite"
        d2 = f32(f32(f32(x * x) + f32(y * y)) + f32(z * z))
        if not (d2 >= rmin2 and d2 <= rmax2):
            return "range"
        if flags is not None and P["drop_flag"] >= 0 and int(flags[k]) == P["drop_flag"]:
            return "flag"
        q = [f32(f32(f32(f32(Rm[i, 0] * x) + f32(Rm[i, 1] * y)) + f32(Rm[i, 2] * z)) + tm[i]) for i in range(3)]
        g = [f32(f32(q[i] - org[i]) / vs) for i in range(3)]
        if not all(g[i] >= zero and g[i] < hi[i] for i in range(3)):
            return "box"
        j = [int(math.floor(float(g[i]))) for i in range(3)]
        f = [f32(g[i] - f32(j[i])) for i in range(3)]
        r00 = j[2] * sz + j[1] * sy + j[0]
        at = {(a, b, c): r00 + c * sz + b * sy + a for a in (0, 1) for b in (0, 1) for c in (0, 1)}
        if not all(w[v] > thr for v in at.values()):
            return "corner"
        c = {key: t[v] for key, v in at.items()}
        d00, d10, d01, d11 = (f32(c[(1, b, cc)] - c[(0, b, cc)]) for cc in (0, 1) for b in (0, 1))
        a00, a10 = f32(c[(0, 0, 0)] + f32(f[0] * d00)), f32(c[(0, 1, 0)] + f32(f[0] * d10))
        a01, a11 = f32(c[(0, 0, 1)] + f32(f[0] * d01)), f32(c[(0, 1, 1)] + f32(f[0] * d11))
        h0, h1 = f32(a10 - a00), f32(a11 - a01)
        b0, b1 = f32(a00 + f32(f[1] * h0)), f32(a01 + f32(f[1] * h1))
        G2 = f32(b1 - b0)
        F = f32(b0 + f32(f[2] * G2))
        e0 = f32(d00 + f32(f[1] * f32(d10 - d00)))
        e1 = f32(d01 + f32(f[1] * f32(d11 - d01)))
        G0 = f32(e0 + f32(f[2] * f32(e1 - e0)))
        G1 = f32(h0 + f32(f[2] * f32(h1 - h0)))
        r = f32(F * tr)
        n = [f32(G0 * gscale), f32(G1 * gscale), f32(G2 * gscale)]
        if not np.isfinite(F):
            return "value"
        if not abs(F) < one:
            return "band"
        if not abs(r) <= rthr:
            return "resid"
        nn = f32(f32(f32(n[0] * n[0]) + f32(n[1] * n[1])) + f32(n[2] * n[2]))
        if not (np.isfinite(n[0]) and np.isfinite(n[1]) and np.isfinite(n[2]) and nn > zero):
            return "normal"
        J = [f32(f32(q[1] * n[2]) - f32(q[2] * n[1])), f32(f32(q[2] * n[0]) - f32(q[0] * n[2])),
             f32(f32(q[0] * n[1]) - f32(q[1] * n[0])), n[0], n[1], n[2]]
        rows.append([f32(J[a] * J[b]) for a, b in UPPER] + [f32(J[a] * r) for a in range(6)] + [f32(r * r), one])
        idx.append(k)
        return None

    with np.errstate(all="ignore"):
        for k in selected(len(pts), level):
            gate = one_point(int(k))
            if gate is not None:
                rejected[gate] += 1
    if info is not None:
        info["idx"] = np.asarray(idx, np.int64)
        info["rejected"] = rejected
    return np.asarray(rows, f32).reshape(-1, N_TERMS)


def system(vol, grid, points, flags, M, level, P, info=None):
    M = np.asarray(M, np.float64).reshape(-1)[:12].reshape(3, 4)
    t64 = pair_terms(vol, grid, points, flags, M[:, :3].astype(f32), M[:, 3].astype(f32), level, P, info).astype(np.float64)
    return t64.sum(axis=0), np.abs(t64).sum(axis=0)


def result_pose(base2world, M):
    """base2world * [M; 0 0 0 1] in double (sums over k left to right), each entry rounded to float32, last row 0 0 0 1."""
    M4 = np.eye(4)
    M4[:3] = np.asarray(M, np.float64)
    out = ts._mul4(np.asarray(base2world, f32).reshape(4, 4).astype(np.float64), M4).astype(f32)
    out[3] = [0, 0, 0, 1]
    return out.ravel()


def track(vol, grid, points, flags, P, guess, history=None):
    """history, a list, receives one dict per iteration that ran: level, pairs, w and tau (|w|, |tau| of the step; None when
    there was none), pivot_ratio (track_spec.cholesky_solve's; None when min_pairs decided), lost, done, near (pair_terms')."""
    guess = np.asarray(guess, f32).ravel().copy()
    M = start_pose(grid, guess)
    lost, done, iters_run, pairs, r2 = False, [0, 0, 0], [0, 0, 0], 0, 0.0
    for lvl in range(P["n_levels"] - 1, -1, -1):
        for _ in range(P["iters"][lvl]):
            if lost or done[lvl]:
                break
            info = {}
            sys, _ = system(vol, grid, points, flags, M, lvl, P, info)
            pairs, r2 = int(sys[28]), float(sys[27])
            iters_run[lvl] += 1
            note = {"level": lvl, "pairs": pairs, "w": None, "tau": None, "pivot_ratio": None, "lost": False, "done": False,
                    "near": info["near"], "selected": info["selected"]}
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
    pose = guess if lost else result_pose(grid[4], M)          # a lost run: the guess's own bits, all 16
    return {"M": M, "velo2world": pose, "status": status, "iters_run": iters_run, "pairs": pairs, "lost": lost,
            "rmse": math.sqrt(r2 / pairs) if pairs > 0 else 0.0}


def pose_error(velo2world, truth):
    """(rotation error in degrees, translation error in metres) of a velo2world against the true one."""
    e_t, e_r = ts.pose_error(velo2world, truth)
    return math.degrees(e_r), e_t
