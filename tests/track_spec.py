"""Float32 NumPy restatement of the tracking rule of csrc/tsdf_track.hip.h (the header comment states it; this follows it line
by line).  Per-sample values are np.float32 evaluated in the header's order, so every pair decision and every per-pair term is
the device's bit for bit; the sums and the solve are float64.  The parity contract, as tests/test_gpu_track_exact.py and
tests/test_gpu_track.py hold it: the system of a single pair equals the double value of these float32 terms exactly (a sum of
one term has no order); a system of n pairs is within n * 2^-52 * sum |term| per entry (np.sum's order is not the device's:
two double sums of the same n terms differ by at most 2 (n - 1) 2^-53 sum |term| to first order) with the pair count exact; a
track's status, iters_run and inliers are equal, its rmse and every entry of its float32 pose within one float32 ulp.

    relative(c_ref, c_cur)                       M [3, 4] float64 = C_ref^-1 * C_cur (rigid inverse), the rule's order
    result_pose(base2world, c_ref, M)            cam2world float32 [16]
    pair_terms(live, model, level, Rm, tm, P)    per-pair terms [n, 29] float32 (info: rejects per gate, the pairs' samples)
    system(live, model, level, M, P)             (sums [29] float64, sum |term| [29] float64)
    track(live, model, P, M0=None)               dict M, status, iters_run, inliers, rmse, lost (history: per iteration)

live = (depth [H, W] float32, mask [H, W] uint8 or None); model = (depth [H, W], normal [H, W, 3]) of the render at C_ref; P: a
dict of the tsdf_track_params fields (params() or from_ctypes()), with K, hw, near, far from its ray member.
"""
import math

import numpy as np

f32 = np.float32
N_TERMS = 29
UPPER = [(a, b) for a in range(6) for b in range(a, 6)]


def params(K, hw, near=0.0, far=6.0, n_levels=3, iters=(10, 5, 4), dist=(0.10, 0.10, 0.10),
           cos_thresh=math.cos(math.radians(20.0)), min_inliers=300, eps_rot=1e-5, eps_trans=1e-5):
    return {"K": np.asarray(K, f32).ravel(), "hw": tuple(hw), "near": f32(near), "far": f32(far), "n_levels": int(n_levels),
            "iters": list(iters), "dist": [f32(x) for x in dist], "cos": f32(cos_thresh), "min_inliers": int(min_inliers),
            "eps_rot": float(f32(eps_rot)), "eps_trans": float(f32(eps_trans))}


def from_ctypes(p):
    """The dict of a capi.TrackParams."""
    return params(np.array(p.ray.cam_K, f32), (p.ray.im_height, p.ray.im_width), p.ray.near_m, p.ray.far_m, p.n_levels,
                  list(p.iters), list(p.dist_thresh), p.cos_normal_thresh, p.min_inliers, p.eps_rot, p.eps_trans)


def relative(c_ref, c_cur):
    r = np.asarray(c_ref, f32).reshape(4, 4).astype(np.float64)
    c = np.asarray(c_cur, f32).reshape(4, 4).astype(np.float64)
    M = np.zeros((3, 4))
    for i in range(3):
        for j in range(3):
            M[i, j] = (r[0, i] * c[0, j] + r[1, i] * c[1, j]) + r[2, i] * c[2, j]
        M[i, 3] = (r[0, i] * (c[0, 3] - r[0, 3]) + r[1, i] * (c[1, 3] - r[1, 3])) + r[2, i] * (c[2, 3] - r[2, 3])
    return M


def _mul4(a, b):
    out = np.zeros((4, 4))
    for i in range(4):
        for j in range(4):
            acc = a[i, 0] * b[0, j]
            for k in range(1, 4):
                acc = acc + a[i, k] * b[k, j]
            out[i, j] = acc
    return out


def result_pose(base2world, c_ref, M):
    X = _mul4(np.asarray(base2world, f32).reshape(4, 4).astype(np.float64),
              np.asarray(c_ref, f32).reshape(4, 4).astype(np.float64))
    M4 = np.eye(4)
    M4[:3] = M
    return _mul4(X, M4).astype(f32).ravel()


def sample_grid(hw, level):
    H, W = hw
    s = 1 << level
    ni = (W - 1 - s) // s + 1 if W > s else 0
    nj = (H - 1 - s) // s + 1 if H > s else 0
    j, i = np.meshgrid(np.arange(nj), np.arange(ni), indexing="ij")
    return s * i.ravel(), s * j.ravel(), s


GATES = ("depth_or_mask", "len", "behind", "off_image", "no_model", "distance", "normal")      # the rule's order


def pair_terms(live, model, level, Rm, tm, P, info=None):
    """(terms [n_pairs, 29] float32, the (u, v) of the pairs).  info, a dict, receives "samples" (ni * nj), "rejected" (a dict
    of GATES: the samples each gate turned away, every sample counted at the first gate that rejects it) and "idx" (the flat
    sample index j * ni + i of every pair, in the order of the terms) and "model_px" (the model pixel (ui, vi) of every pair)."""
    depth, mask = live
    mdepth, mnormal = model
    depth = np.asarray(depth, f32)
    H, W = P["hw"]
    K = P["K"]
    fx, fy, cx, cy = K[0], K[4], K[2], K[5]
    near, far = P["near"], P["far"]
    Rm = np.asarray(Rm, f32).reshape(3, 3)
    tm = np.asarray(tm, f32).ravel()
    u, v, s = sample_grid((H, W), level)
    left = [u.size]                                    # samples still alive after each gate

    def ok(d, uu, vv):
        with np.errstate(invalid="ignore"):
            g = np.isfinite(d) & (near < d) & (d <= far)
        if mask is not None:
            g &= np.asarray(mask)[vv, uu] >= 128
        return g

    d00, d10, d01 = depth[v, u], depth[v, u + s], depth[v + s, u]
    keep = ok(d00, u, v) & ok(d10, u + s, v) & ok(d01, u, v + s)
    u, v, d00, d10, d01 = u[keep], v[keep], d00[keep], d10[keep], d01[keep]
    left.append(u.size)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        dcx0 = (u.astype(f32) - cx) / fx
        dcx1 = ((u + s).astype(f32) - cx) / fx
        dcy0 = (v.astype(f32) - cy) / fy
        dcy1 = ((v + s).astype(f32) - cy) / fy
        V = [d00 * dcx0, d00 * dcy0, d00]
        a = [d10 * dcx1 - V[0], d10 * dcy0 - V[1], d10 - V[2]]
        b = [d01 * dcx0 - V[0], d01 * dcy1 - V[1], d01 - V[2]]
        n = [b[1] * a[2] - b[2] * a[1], b[2] * a[0] - b[0] * a[2], b[0] * a[1] - b[1] * a[0]]
        ln = np.sqrt((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2])
        keep = np.isfinite(ln) & (ln > f32(0))
        left.append(int(keep.sum()))
        n = [x / ln for x in n]
        Pp = [((Rm[k, 0] * V[0] + Rm[k, 1] * V[1]) + Rm[k, 2] * V[2]) + tm[k] for k in range(3)]
        nl = [(Rm[k, 0] * n[0] + Rm[k, 1] * n[1]) + Rm[k, 2] * n[2] for k in range(3)]
        keep &= Pp[2] > f32(0)
        left.append(int(keep.sum()))
        pu = fx * (Pp[0] / Pp[2]) + cx
        pv = fy * (Pp[1] / Pp[2]) + cy
        keep &= np.isfinite(pu) & np.isfinite(pv) & (pu >= f32(-0.5)) & (pu < f32(W) - f32(0.5)) & \
            (pv >= f32(-0.5)) & (pv < f32(H) - f32(0.5))
        fu = np.floor(np.where(keep, pu, f32(0)) + f32(0.5))
        fv = np.floor(np.where(keep, pv, f32(0)) + f32(0.5))
    ui, vi = fu.astype(np.int64), fv.astype(np.int64)
    keep &= (ui >= 0) & (ui < W) & (vi >= 0) & (vi < H)
    left.append(int(keep.sum()))
    ui, vi = np.where(keep, ui, 0), np.where(keep, vi, 0)
    t = np.asarray(mdepth, f32)[vi, ui]
    nm = np.asarray(mnormal, f32)[vi, ui]
    nm = [nm[:, 0], nm[:, 1], nm[:, 2]]
    keep &= (t > f32(0)) & ~((nm[0] == 0) & (nm[1] == 0) & (nm[2] == 0))
    left.append(int(keep.sum()))
    dist2 = P["dist"][level] * P["dist"][level]
    with np.errstate(invalid="ignore", over="ignore"):
        q = [t * ((ui.astype(f32) - cx) / fx), t * ((vi.astype(f32) - cy) / fy), t]
        e = [Pp[k] - q[k] for k in range(3)]
        keep &= ((e[0] * e[0] + e[1] * e[1]) + e[2] * e[2]) <= dist2
        left.append(int(keep.sum()))
        keep &= ((nl[0] * nm[0] + nl[1] * nm[1]) + nl[2] * nm[2]) >= P["cos"]
        sel = lambda x: x[keep]
        e, nm, Pp = [sel(x) for x in e], [sel(x) for x in nm], [sel(x) for x in Pp]
        r = (nm[0] * e[0] + nm[1] * e[1]) + nm[2] * e[2]
        J = [Pp[1] * nm[2] - Pp[2] * nm[1], Pp[2] * nm[0] - Pp[0] * nm[2], Pp[0] * nm[1] - Pp[1] * nm[0], nm[0], nm[1], nm[2]]
        cols = [J[a] * J[b] for a, b in UPPER] + [J[a] * r for a in range(6)] + [r * r, np.ones_like(r)]
    if info is not None:
        left.append(int(keep.sum()))
        ni = (W - 1 - s) // s + 1 if W > s else 0
        info["samples"] = left[0]
        info["rejected"] = {g: left[k] - left[k + 1] for k, g in enumerate(GATES)}
        info["idx"] = (v[keep] // s) * ni + u[keep] // s
        info["model_px"] = (ui[keep], vi[keep])
    return np.stack(cols, axis=1).astype(f32), (u[keep], v[keep])


def system(live, model, level, M, P):
    M = np.asarray(M, np.float64)
    terms, _ = pair_terms(live, model, level, M[:, :3].astype(f32), M[:, 3].astype(f32), P)
    t64 = terms.astype(np.float64)
    return t64.sum(axis=0), np.abs(t64).sum(axis=0)


def unpack(sys):
    A = np.zeros((6, 6))
    A[np.triu_indices(6)] = sys[:21]
    A = A + np.triu(A, 1).T
    return A, np.asarray(sys[21:27]), float(sys[27]), float(sys[28])


def cholesky_solve(sys, info=None):
    """xi of A xi = -b, or None when a pivot is <= 1e-12 * max diagonal (the rule's loop, in double).  info, a dict, receives
    "pivot_ratio": the smallest pivot met over 1e-12 * max diagonal (<= 1 exactly when lost; 0 for an all-zero diagonal)."""
    A, b, _, _ = unpack(sys)
    dmax = max(A[a, a] for a in range(6))
    L = np.zeros((6, 6))
    ratio = math.inf
    for c in range(6):
        piv = A[c, c]
        for j in range(c):
            piv -= L[c, j] * L[c, j]
        ratio = min(ratio, piv / (1e-12 * dmax) if dmax > 0.0 else 0.0)
        if info is not None:
            info["pivot_ratio"] = ratio
        if not piv > 1e-12 * dmax:
            return None
        L[c, c] = math.sqrt(piv)
        for rr in range(c + 1, 6):
            x = A[rr, c]
            for j in range(c):
                x -= L[rr, j] * L[c, j]
            L[rr, c] = x / L[c, c]
    y = np.zeros(6)
    for a in range(6):
        x = -b[a]
        for j in range(a):
            x -= L[a, j] * y[j]
        y[a] = x / L[a, a]
    xi = np.zeros(6)
    for a in range(5, -1, -1):
        x = y[a]
        for j in range(a + 1, 6):
            x -= L[j, a] * xi[j]
        xi[a] = x / L[a, a]
    return xi


def rodrigues(w):
    th = math.sqrt((w[0] * w[0] + w[1] * w[1]) + w[2] * w[2])
    if th == 0.0:
        return np.eye(3)
    k = np.asarray(w, np.float64) / th
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return (np.eye(3) + math.sin(th) * Kx) + (1.0 - math.cos(th)) * (Kx @ Kx)


def step(M, xi):
    """[Rodrigues(w) | tau] * M in the device's order of operations (sums over k left to right, no contraction)."""
    w = [float(x) for x in xi[:3]]
    th = math.sqrt((w[0] * w[0] + w[1] * w[1]) + w[2] * w[2])
    R = [[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]]
    if th > 0.0:
        kx, ky, kz = w[0] / th, w[1] / th, w[2] / th
        sn, cs = math.sin(th), 1.0 - math.cos(th)
        Kx = [[0.0, -kz, ky], [kz, 0.0, -kx], [-ky, kx, 0.0]]
        for a in range(3):
            for b in range(3):
                k2 = (Kx[a][0] * Kx[0][b] + Kx[a][1] * Kx[1][b]) + Kx[a][2] * Kx[2][b]
                R[a][b] = (R[a][b] + sn * Kx[a][b]) + cs * k2
    out = np.zeros((3, 4))
    for a in range(3):
        for b in range(3):
            out[a, b] = (R[a][0] * M[0, b] + R[a][1] * M[1, b]) + R[a][2] * M[2, b]
        out[a, 3] = ((R[a][0] * M[0, 3] + R[a][1] * M[1, 3]) + R[a][2] * M[2, 3]) + float(xi[3 + a])
    return out


def track(live, model, P, M0=None, history=None):
    """history, a list, receives one dict per iteration that ran: level, pairs, w and tau (|w|, |tau| of the step; None when
    there was none), pivot_ratio (cholesky_solve's; None when min_inliers decided), lost, done."""
    M = np.hstack([np.eye(3), np.zeros((3, 1))]) if M0 is None else np.asarray(M0, np.float64).copy()
    lost, done, iters_run, inliers, r2 = False, [0, 0, 0], [0, 0, 0], 0, 0.0
    for lvl in range(P["n_levels"] - 1, -1, -1):
        for _ in range(P["iters"][lvl]):
            if lost or done[lvl]:
                break
            sys, _ = system(live, model, lvl, M, P)
            inliers, r2 = int(sys[28]), float(sys[27])
            iters_run[lvl] += 1
            note = {"level": lvl, "pairs": inliers, "w": None, "tau": None, "pivot_ratio": None, "lost": False, "done": False}
            if history is not None:
                history.append(note)
            xi = cholesky_solve(sys, note) if sys[28] >= P["min_inliers"] else None
            if xi is None:
                lost = note["lost"] = True
                break
            M = step(M, xi)
            th = math.sqrt((xi[0] * xi[0] + xi[1] * xi[1]) + xi[2] * xi[2])
            tn = math.sqrt((xi[3] * xi[3] + xi[4] * xi[4]) + xi[5] * xi[5])
            note["w"], note["tau"] = th, tn
            if th < P["eps_rot"] and tn < P["eps_trans"]:
                done[lvl] = 1
                note["done"] = True
    ran = [lvl for lvl in range(P["n_levels"]) if P["iters"][lvl] > 0]
    status = 2 if lost else (0 if ran and done[ran[0]] else 1)
    return {"M": M, "status": status, "iters_run": iters_run, "inliers": inliers, "lost": lost,
            "rmse": math.sqrt(r2 / inliers) if inliers > 0 else 0.0}


def pose_error(a, b):
    """(translation error in metres, rotation error in radians) between two 4 x 4 poses."""
    A = np.asarray(a, np.float64).reshape(4, 4)
    B = np.asarray(b, np.float64).reshape(4, 4)
    dR = A[:3, :3].T @ B[:3, :3]
    sn = 0.5 * math.sqrt((dR[2, 1] - dR[1, 2]) ** 2 + (dR[0, 2] - dR[2, 0]) ** 2 + (dR[1, 0] - dR[0, 1]) ** 2)
    ang = math.atan2(sn, (np.trace(dR) - 1.0) / 2.0)          # (acos of the trace alone loses small angles)
    return float(np.linalg.norm(A[:3, 3] - B[:3, 3])), ang


def perturb(pose, rng, max_deg=3.0, max_m=0.03):
    """pose moved by a rotation of up to max_deg about a random axis (about the camera centre) and a shift of up to max_m in
    a random direction; returns float32 [16]."""
    T = np.asarray(pose, np.float64).reshape(4, 4).copy()
    ax = rng.normal(size=3)
    ax /= np.linalg.norm(ax)
    ang = math.radians(rng.uniform(0.5, 1.0) * max_deg)
    d = rng.normal(size=3)
    d /= np.linalg.norm(d)
    T[:3, :3] = rodrigues(ax * ang) @ T[:3, :3]
    T[:3, 3] += d * rng.uniform(0.5, 1.0) * max_m
    return T.astype(f32).ravel()
