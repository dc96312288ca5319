"""Float32 NumPy restatement of the raycasting rule of csrc/tsdf_raycast.hip.h (the header comment states it; this follows it
line by line).  Every value is np.float32 and every operation is evaluated in the header's order, so the device matches this
bit for bit.  Vectorised over rays: the march advances all rays that are still active by one sample per iteration.

    render(tsdf, weight, dims, origin, vs, trunc, K, hw, near, far, weight_thresh, cam2base, pixels=None, label=None,
           colour=None)

tsdf / weight: flat x-fastest float32 arrays of the whole grid; pixels: None (every pixel, row-major) or an int array [n, 2] of
(u, v).  Returns a dict of "depth" [n], "normal" [n, 3], "hit" [n] bool, "samples" [n] (samples taken per ray), and "label" /
"colour" [n] when those arrays are given.  With report=True it also says how each ray ended and what its set-up was: "end" [n]
(an index into END), "go" [3], "gd" [n, 3], "gd_zero" [n, 3] (gd_i == 0), "touch" [n] (t_enter == t_exit on a ray that passed the
set-up), "t_enter" / "t_exit" [n], "g_hit" [n, 3] (g* of the rule), and "trace": the march's samples as "t", "F" [k, n] float32 and "valid" [k, n] bool (rows past a ray's last sample
hold NaN / False).  The report reads the arithmetic; it takes no part in it.
"""
import numpy as np

f32 = np.float32
END = ("setup_miss", "hit", "exit", "stall", "cap")


def max_steps(dims):
    return 2 * (int(dims[0]) + int(dims[1]) + int(dims[2])) + 8


def pose_parts(cam2base, origin, vs):
    """R [3, 3], go [3] of the rule (go = (T - origin) / vs, float32)."""
    c = np.asarray(cam2base, f32).reshape(4, 4)
    R = np.ascontiguousarray(c[:3, :3])
    with np.errstate(invalid="ignore", over="ignore"):                        # a go that is not finite is a miss, by the rule
        go = (c[:3, 3] - np.asarray(origin, f32)) / f32(vs)
    return R, go.astype(f32)


def sample(tsdf, weight, dims, wthr, g):
    """(valid [n], F [n]) at grid points g [3, n]."""
    dims = [int(d) for d in dims]
    hi = [f32(d - 1) for d in dims]
    with np.errstate(invalid="ignore"):
        inside = np.ones(g.shape[1], bool)
        for i in range(3):
            inside &= (g[i] >= f32(0)) & (g[i] <= hi[i])
    gc = [np.where(inside, g[i], f32(0)) for i in range(3)]          # out-of-range rays read voxel 0 and are invalid anyway
    j = [np.minimum(np.floor(gc[i]).astype(np.int64), dims[i] - 2) for i in range(3)]
    f = [(gc[i] - j[i].astype(f32)).astype(f32) for i in range(3)]
    sy, sz = dims[0], dims[0] * dims[1]
    b = j[2] * sz + j[1] * sy + j[0]
    offs = [0, 1, sy, sy + 1, sz, sz + 1, sz + sy, sz + sy + 1]
    c = [tsdf[b + o] for o in offs]
    wok = np.ones(g.shape[1], bool)
    with np.errstate(invalid="ignore"):
        for o in offs:
            wok &= weight[b + o] > wthr
    c000, c100, c010, c110, c001, c101, c011, c111 = c
    with np.errstate(invalid="ignore", over="ignore"):
        a00 = c000 + f[0] * (c100 - c000)
        a10 = c010 + f[0] * (c110 - c010)
        a01 = c001 + f[0] * (c101 - c001)
        a11 = c011 + f[0] * (c111 - c011)
        b0 = a00 + f[1] * (a10 - a00)
        b1 = a01 + f[1] * (a11 - a01)
        F = b0 + f[2] * (b1 - b0)
    return inside & wok & np.isfinite(F), F.astype(f32)


def render(tsdf, weight, dims, origin, vs, trunc, K, hw, near, far, weight_thresh, cam2base, pixels=None, label=None,
           colour=None, report=False):
    tsdf = np.ascontiguousarray(tsdf, f32).ravel()
    weight = np.ascontiguousarray(weight, f32).ravel()
    dims = [int(d) for d in dims]
    hi = [f32(d - 1) for d in dims]
    K = np.asarray(K, f32).ravel()
    fx, fy, cx, cy = K[0], K[4], K[2], K[5]
    vs, s_free = f32(vs), f32(0.8) * f32(trunc)
    near, far, wthr = f32(near), f32(far), f32(weight_thresh)
    if pixels is None:
        h, w = hw
        vv, uu = np.mgrid[0:h, 0:w]
        u, v = uu.ravel(), vv.ravel()
    else:
        pixels = np.asarray(pixels)
        u, v = pixels[:, 0], pixels[:, 1]
    n = u.size
    R, go = pose_parts(cam2base, origin, vs)
    dcx = (u.astype(f32) - cx) / fx
    dcy = (v.astype(f32) - cy) / fy
    r = f32(1) / np.sqrt((dcx * dcx + dcy * dcy) + f32(1))
    gd = np.empty((3, n), f32)
    ok = np.ones(n, bool)
    t_enter = np.full(n, near, f32)
    t_exit = np.full(n, far, f32)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        for i in range(3):
            db = (R[i, 0] * dcx + R[i, 1] * dcy) + R[i, 2]
            gd[i] = db / vs
            ok &= np.isfinite(go[i]) & np.isfinite(gd[i])
            zero = gd[i] == f32(0)
            ok &= ~zero | ((go[i] >= f32(0)) & (go[i] <= hi[i]))
            a = (f32(0) - go[i]) / gd[i]
            b = (hi[i] - go[i]) / gd[i]
            lo = np.where(a < b, a, b)
            up = np.where(a < b, b, a)
            t_enter = np.where(~zero & (lo > t_enter), lo, t_enter)
            t_exit = np.where(~zero & (up < t_exit), up, t_exit)
        ok &= t_enter <= t_exit

    t = t_enter.copy()
    t_prev = np.zeros(n, f32)
    F_prev = np.zeros(n, f32)
    prev_valid = np.zeros(n, bool)
    active = ok.copy()
    hit = np.zeros(n, bool)
    ts = np.zeros(n, f32)
    samples = np.zeros(n, np.int64)
    end = np.where(ok, END.index("cap"), END.index("setup_miss"))      # a ray still active after the last sample met the cap
    trace = {"t": [], "F": [], "valid": []}
    for _ in range(max_steps(dims)):
        idx = np.nonzero(active)[0]
        if idx.size == 0:
            break
        tt = t[idx]
        with np.errstate(invalid="ignore", over="ignore"):
            g = np.stack([go[i] + tt * gd[i, idx] for i in range(3)])
        valid, F = sample(tsdf, weight, dims, wthr, g)
        samples[idx] += 1
        if report:
            for key, val, fill in (("t", tt, np.nan), ("F", F, np.nan), ("valid", valid, False)):
                row = np.full(n, fill, val.dtype)
                row[idx] = val
                trace[key].append(row)
        h = valid & prev_valid[idx] & (F_prev[idx] > f32(0)) & (F <= f32(0))
        hi_idx = idx[h]
        fp, tp = F_prev[hi_idx], t_prev[hi_idx]
        ts[hi_idx] = tp + (tt[h] - tp) * (fp / (fp - F[h]))
        hit[hi_idx] = True
        active[hi_idx] = False
        end[hi_idx] = END.index("hit")
        go_on = ~h
        idx, tt, valid, F = idx[go_on], tt[go_on], valid[go_on], F[go_on]
        with np.errstate(invalid="ignore", over="ignore"):
            step = np.where(valid, np.where(F > f32(0), np.fmax(vs, s_free * F), vs), s_free).astype(f32)
            tn = tt + step * r[idx]
        stall = ~(tn > tt)
        active[idx[stall]] = False
        end[idx[stall]] = END.index("stall")
        keep = ~stall
        idx, tt, valid, F, tn = idx[keep], tt[keep], valid[keep], F[keep], tn[keep]
        t_prev[idx] = tt
        F_prev[idx] = F
        prev_valid[idx] = valid
        t[idx] = tn
        active[idx[~(tn <= t_exit[idx])]] = False
        end[idx[~(tn <= t_exit[idx])]] = END.index("exit")

    out = {"hit": hit, "samples": samples, "depth": np.where(hit, ts, f32(0)).astype(f32)}
    with np.errstate(invalid="ignore", over="ignore"):
        gs = np.stack([go[i] + ts * gd[i] for i in range(3)])
    if report:
        with np.errstate(invalid="ignore"):
            out.update(end=end, go=go, gd=gd.T, gd_zero=(gd == f32(0)).T, touch=ok & (t_enter == t_exit), t_enter=t_enter,
                       t_exit=t_exit, g_hit=gs.T,
                       trace={k: np.stack(v) if v else np.zeros((0, n), bool if k == "valid" else f32)
                              for k, v in trace.items()})
    normal = np.zeros((n, 3), f32)
    hidx = np.nonzero(hit)[0]
    if hidx.size:
        gh = gs[:, hidx]
        nn = []
        okn = np.ones(hidx.size, bool)
        for i in range(3):
            p, q = gh.copy(), gh.copy()
            p[i] = gh[i] + f32(1)
            q[i] = gh[i] - f32(1)
            vp, Fp = sample(tsdf, weight, dims, wthr, p)
            vq, Fq = sample(tsdf, weight, dims, wthr, q)
            okn &= vp & vq
            with np.errstate(invalid="ignore", over="ignore"):
                nn.append(Fp - Fq)
        with np.errstate(invalid="ignore", over="ignore", divide="ignore"):   # len == 0: m / len is computed and dropped
            m = [(R[0, j] * nn[0] + R[1, j] * nn[1]) + R[2, j] * nn[2] for j in range(3)]
            ln = np.sqrt((m[0] * m[0] + m[1] * m[1]) + m[2] * m[2])
            okn &= np.isfinite(ln) & (ln > f32(0))
            for j in range(3):
                normal[hidx, j] = np.where(okn, m[j] / ln, f32(0))
    out["normal"] = normal
    if label is not None or colour is not None:
        c = []
        with np.errstate(invalid="ignore"):
            for i in range(3):
                x = np.floor(gs[i] + f32(0.5))
                x = np.where(x < f32(0), f32(0), x)
                x = np.where(x > hi[i], hi[i], x)
                c.append(np.where(hit, x, f32(0)).astype(np.int64))
        vox = (c[2] * dims[1] + c[1]) * dims[0] + c[0]
        if label is not None:
            out["label"] = np.where(hit, np.asarray(label).ravel()[vox], 0).astype(np.uint16)
        if colour is not None:
            out["colour"] = np.where(hit, np.asarray(colour).ravel()[vox], 0).astype(np.uint32)
    return out


def render_batch(members, K, hw, near, far, weight_thresh, pixels=None, report=False):
    """members: list of dicts with the render() arguments tsdf, weight, dims, origin, vs, trunc, cam2base.  Per pixel the
    nearest hit wins, ties to the lower index.  Returns depth, normal, member (-1 = miss); with report=True also "members",
    each member's own render(report=True)."""
    outs = [render(m["tsdf"], m["weight"], m["dims"], m["origin"], m["vs"], m["trunc"], K, hw, near, far, weight_thresh,
                   m["cam2base"], pixels=pixels, report=report) for m in members]
    d = np.stack([np.where(o["hit"], o["depth"], np.inf) for o in outs])
    who = np.argmin(d, axis=0)
    anyhit = np.isfinite(d.min(axis=0))
    n = d.shape[1]
    depth = np.where(anyhit, d[who, np.arange(n)], 0).astype(f32)
    normal = np.stack([o["normal"] for o in outs])[who, np.arange(n)]
    normal = np.where(anyhit[:, None], normal, f32(0)).astype(f32)
    out = {"depth": depth, "normal": normal, "member": np.where(anyhit, who, -1).astype(np.int32)}
    if report:
        out["members"] = outs
    return out
