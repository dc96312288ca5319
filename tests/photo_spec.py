"""Float32 NumPy restatement of the photometric tracking rule of csrc/tsdf_photo.hip.h (the header comment states it; this
follows it line by line).  Per-sample values are np.float32 evaluated in the header's order, so every pair decision and every
per-pair term is the device's bit for bit; the sums and the solve are float64.  The parity contract is track_spec's: a single
pair's system equals the double value of these float32 terms, a system of n pairs is within n * 2^-52 * sum |term| per entry
with the count exact, a track's integers are equal and its float32 results within one ulp.

    luma(r, g, b), luma_packed(colour)               float32 intensities in [0, 1]
    model_intensity(mdepth, colour, weight, dims, origin, vs, ray, cam2base)     level 0 of the model pyramid [H, W]
    halve(I), pyramid(I0, n_levels)                  the 2 x 2 mean with validity; the list of levels
    live_pyramid(rgb, n_levels)
    pair_terms(live, model, level, Rm, tm, P, PP, info=None)      per-pair terms [n, 29] float32
    system(live, model, level, M, P, PP)             (sums [29] float64, sum |term| [29] float64)
    track(live, model, P, PP, M0=None, history=None) track_spec.track's dict plus photo_pairs, photo_rmse, photo_r2

live = (depth [H, W] float32, mask [H, W] uint8 or None, live pyramid or None); model = (depth [H, W], normal [H, W, 3], model
pyramid or None) of the render at C_ref; P: track_spec's dict; PP: {"weight": photo_weight, "ithr": intensity_thresh}; ray:
{"K", "hw", "near", "far", "wthr"}.  Invalid intensities are -1."""
import math

import numpy as np

import raycast_spec as rs
import track_spec as ts

f32 = np.float32
N_LEVELS = 3
INVALID = f32(-1.0)
DEFAULT_WEIGHT, DEFAULT_ITHR = 0.1, 0.25      # tsdf_photo_params_default
GATES = ("depth_or_mask", "behind", "off_image", "footprint", "invalid_intensity", "occluded", "residual")   # the rule's order


def photo_params(weight=DEFAULT_WEIGHT, ithr=DEFAULT_ITHR):
    return {"weight": f32(weight), "ithr": f32(ithr)}


def luma(r, g, b):
    r, g, b = (np.asarray(x).astype(f32) for x in (r, g, b))
    return (((f32(0.299) * r + f32(0.587) * g) + f32(0.114) * b) / f32(255.0)).astype(f32)


def luma_packed(colour):
    c = np.asarray(colour, np.uint32)
    return luma(c & 255, (c >> 8) & 255, (c >> 16) & 255)


def model_intensity(mdepth, colour, weight, dims, origin, vs, ray, cam2base):
    """Level 0 of the model pyramid from the depth render mdepth [H, W] at cam2base (the rule's Model)."""
    H, W = ray["hw"]
    K = np.asarray(ray["K"], f32).ravel()
    fx, fy, cx, cy = K[0], K[4], K[2], K[5]
    t = np.asarray(mdepth, f32).reshape(H * W)
    vv, uu = np.mgrid[0:H, 0:W]
    u, v = uu.ravel(), vv.ravel()
    R, go = rs.pose_parts(cam2base, origin, vs)
    dcx = (u.astype(f32) - cx) / fx
    dcy = (v.astype(f32) - cy) / fy
    hit = t > f32(0)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        g = []
        for i in range(3):
            db = (R[i, 0] * dcx + R[i, 1] * dcy) + R[i, 2]
            gd = db / f32(vs)
            g.append(np.where(hit, go[i] + t * gd, f32(-1)).astype(f32))
    y = luma_packed(np.asarray(colour, np.uint32).ravel())
    valid, I = rs.sample(y, np.ascontiguousarray(weight, f32).ravel(), dims, f32(ray["wthr"]), np.stack(g))
    return np.where(hit & valid, I, INVALID).astype(f32).reshape(H, W)


def halve(I):
    I = np.asarray(I, f32)
    Ho, Wo = I.shape[0] // 2, I.shape[1] // 2
    I00, I10 = I[0:2 * Ho:2, 0:2 * Wo:2], I[0:2 * Ho:2, 1:2 * Wo:2]
    I01, I11 = I[1:2 * Ho:2, 0:2 * Wo:2], I[1:2 * Ho:2, 1:2 * Wo:2]
    ok = (I00 >= 0) & (I10 >= 0) & (I01 >= 0) & (I11 >= 0)
    return np.where(ok, ((I00 + I10) + (I01 + I11)) * f32(0.25), INVALID).astype(f32)


def pyramid(I0, n_levels=N_LEVELS):
    out = [np.asarray(I0, f32)]
    for _ in range(1, n_levels):
        out.append(halve(out[-1]))
    return out


def live_pyramid(rgb, n_levels=N_LEVELS):
    rgb = np.asarray(rgb, np.uint8)
    return pyramid(luma(rgb[..., 0], rgb[..., 1], rgb[..., 2]), n_levels)


def pair_terms(live, model, level, Rm, tm, P, PP, info=None):
    """(terms [n_pairs, 29] float32, the (u, v) of the pairs).  info, a dict, receives "samples", "rejected" (a dict of GATES,
    every sample counted at the first gate that rejects it), "idx" (flat sample index of every pair), "r", "J" and
    "footprint_sides" (the samples the footprint gate turned away, per side of the level image it left)."""
    depth, mask, lpyr = live
    mdepth, mpyr = model[0], model[-1]
    depth = np.asarray(depth, f32)
    H, W = P["hw"]
    K = P["K"]
    fx, fy, cx, cy = K[0], K[4], K[2], K[5]
    near, far = P["near"], P["far"]
    Rm = np.asarray(Rm, f32).reshape(3, 3)
    tm = np.asarray(tm, f32).ravel()
    u, v, s = ts.sample_grid((H, W), level)
    ni = (W - 1 - s) // s + 1 if W > s else 0
    L_img, M_img = np.asarray(lpyr[level], f32), np.asarray(mpyr[level], f32)
    Hl, Wl = H >> level, W >> level
    assert M_img.shape == (Hl, Wl) and L_img.shape == (Hl, Wl)
    left = [u.size]
    h, fs = f32(s - 1) * f32(0.5), f32(s)
    d = depth[v, u] if u.size else np.zeros(0, f32)
    with np.errstate(invalid="ignore"):
        keep = np.isfinite(d) & (near < d) & (d <= far)
    if mask is not None and u.size:
        keep &= np.asarray(mask)[v, u] >= 128
    u, v, d = u[keep], v[keep], d[keep]
    left.append(u.size)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        dcx = ((u.astype(f32) + h) - cx) / fx
        dcy = ((v.astype(f32) + h) - cy) / fy
        V = [d * dcx, d * dcy, d]
        Pp = [((Rm[k, 0] * V[0] + Rm[k, 1] * V[1]) + Rm[k, 2] * V[2]) + tm[k] for k in range(3)]
        keep = Pp[2] > f32(0)
        left.append(int(keep.sum()))
        pu = fx * (Pp[0] / Pp[2]) + cx
        pv = fy * (Pp[1] / Pp[2]) + cy
        keep &= np.isfinite(pu) & np.isfinite(pv) & (pu >= f32(-0.5)) & (pu < f32(W) - f32(0.5)) & \
            (pv >= f32(-0.5)) & (pv < f32(H) - f32(0.5))
        pu, pv = np.where(keep, pu, f32(0)), np.where(keep, pv, f32(0))
        ui = np.floor(pu + f32(0.5)).astype(np.int64)
        vi = np.floor(pv + f32(0.5)).astype(np.int64)
        keep &= (ui >= 0) & (ui < W) & (vi >= 0) & (vi < H)
        left.append(int(keep.sum()))
        ui, vi = np.where(keep, ui, 0), np.where(keep, vi, 0)
        x, y = (pu - h) / fs, (pv - h) / fs
        x0, y0 = np.floor(x), np.floor(y)
        before = keep.copy()
        keep &= (x0 >= f32(0)) & (x0 + f32(1) <= f32(Wl - 1)) & (y0 >= f32(0)) & (y0 + f32(1) <= f32(Hl - 1))
        left.append(int(keep.sum()))
        sides = {"left": x0 < f32(0), "right": x0 + f32(1) > f32(Wl - 1), "top": y0 < f32(0), "bottom": y0 + f32(1) > f32(Hl - 1)}
        sides = {k: int((m & before & ~keep).sum()) for k, m in sides.items()}
        xi, yi = np.where(keep, x0, 0).astype(np.int64), np.where(keep, y0, 0).astype(np.int64)
        if Wl >= 2 and Hl >= 2:
            I00, I10, I01, I11 = M_img[yi, xi], M_img[yi, xi + 1], M_img[yi + 1, xi], M_img[yi + 1, xi + 1]
            Lv = L_img[v // s, u // s]
        else:
            I00 = I10 = I01 = I11 = Lv = np.full(u.size, INVALID, f32)
        keep &= (I00 >= 0) & (I10 >= 0) & (I01 >= 0) & (I11 >= 0) & (Lv >= 0)
        left.append(int(keep.sum()))
        t = np.asarray(mdepth, f32)[vi, ui]
        keep &= (t > f32(0)) & (np.abs(Pp[2] - t) <= P["dist"][level])
        left.append(int(keep.sum()))
        ax, ay = x - x0, y - y0
        top = I00 + ax * (I10 - I00)
        bot = I01 + ax * (I11 - I01)
        Im = top + ay * (bot - top)
        r = Im - Lv
        keep &= np.abs(r) <= PP["ithr"]
        left.append(int(keep.sum()))
        gx = (f32(1) - ay) * (I10 - I00) + ay * (I11 - I01)
        gy = (f32(1) - ax) * (I01 - I00) + ax * (I11 - I10)
        a, b = (fx * gx) / fs, (fy * gy) / fs
        sel = lambda z: z[keep]
        a, b, r, Pp = sel(a), sel(b), sel(r), [sel(z) for z in Pp]
        Jp = [a / Pp[2], b / Pp[2], -(((a * Pp[0] + b * Pp[1]) / Pp[2]) / Pp[2])]
        J = [Pp[1] * Jp[2] - Pp[2] * Jp[1], Pp[2] * Jp[0] - Pp[0] * Jp[2], Pp[0] * Jp[1] - Pp[1] * Jp[0], Jp[0], Jp[1], Jp[2]]
        cols = [J[p] * J[q] for p, q in ts.UPPER] + [J[p] * r for p in range(6)] + [r * r, np.ones_like(r)]
    if info is not None:
        info["samples"] = left[0]
        info["rejected"] = {g: left[k] - left[k + 1] for k, g in enumerate(GATES)}
        info["idx"] = (v[keep] // s) * ni + u[keep] // s
        info["r"], info["J"] = r, np.stack(J, axis=1) if r.size else np.zeros((0, 6), f32)
        info["footprint_sides"] = sides
    return np.stack(cols, axis=1).astype(f32), (u[keep], v[keep])


def system(live, model, level, M, P, PP):
    M = np.asarray(M, np.float64)
    terms, _ = pair_terms(live, model, level, M[:, :3].astype(f32), M[:, 3].astype(f32), P, PP)
    t64 = terms.astype(np.float64)
    return t64.sum(axis=0), np.abs(t64).sum(axis=0)


def combine(geo, pho, PP):
    """The combined system of the rule's Solve: entries 0..26 g + lam2 * p, sum r^2 and count the geometric ones."""
    lam2 = float(PP["weight"]) * float(PP["weight"])
    out = np.array(geo, np.float64)
    out[:27] = out[:27] + lam2 * np.asarray(pho, np.float64)[:27]
    return out


def photo_cost(live, model, level, M, P, PP):
    """(sum r^2, pairs) of the photometric term at M."""
    s, _ = system(live, model, level, M, P, PP)
    return float(s[27]), int(s[28])


def track(live, model, P, PP, M0=None, history=None):
    """track_spec.track with the combined system; without a live pyramid or with photo_weight 0 it IS track_spec.track."""
    if live[2] is None or float(PP["weight"]) == 0.0:
        r = ts.track((live[0], live[1]), (model[0], model[1]), P, M0, history)
        r.update(photo_pairs=0, photo_rmse=0.0, photo_r2=0.0)
        return r
    M = np.hstack([np.eye(3), np.zeros((3, 1))]) if M0 is None else np.asarray(M0, np.float64).copy()
    lost, done, iters_run, inliers, r2, pp, pr2 = False, [0, 0, 0], [0, 0, 0], 0, 0.0, 0, 0.0
    for lvl in range(P["n_levels"] - 1, -1, -1):
        for _ in range(P["iters"][lvl]):
            if lost or done[lvl]:
                break
            geo, _ = ts.system((live[0], live[1]), (model[0], model[1]), lvl, M, P)
            pho, _ = system(live, model, lvl, M, P, PP)
            inliers, r2, pp, pr2 = int(geo[28]), float(geo[27]), int(pho[28]), float(pho[27])
            iters_run[lvl] += 1
            note = {"level": lvl, "pairs": inliers, "photo_pairs": pp, "w": None, "tau": None, "pivot_ratio": None, "lost": False,
                    "done": False}
            if history is not None:
                history.append(note)
            xi = ts.cholesky_solve(combine(geo, pho, PP), note) if geo[28] >= P["min_inliers"] else None
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
    return {"M": M, "status": status, "iters_run": iters_run, "inliers": inliers, "lost": lost,
            "rmse": math.sqrt(r2 / inliers) if inliers > 0 else 0.0, "photo_pairs": pp, "photo_r2": pr2,
            "photo_rmse": math.sqrt(pr2 / pp) if pp > 0 else 0.0}
