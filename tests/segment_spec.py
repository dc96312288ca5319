"""NumPy restatement of the geometric segmentation and mask refinement rule of csrc/tsdf_segment.hip.h and include/tsdf_hip.h
(tsdf_segment_depth_device / tsdf_segment_refine_masks_device / tsdf_segment_frame).

Every operation is one the device rounds the same way: float32 + - * / in the order written, integer arithmetic, and double
+ - * / sqrt for the covariance and the Jacobi sweeps; every sum is an integer sum.  So the DoN image, the cluster image, the
count block and the refined masks equal the device's bit for bit."""
import numpy as np

f32 = np.float32
f64 = np.float64
T = 8                      # lattice half-width: (2T + 1)^2 = 289 taps per radius
SWEEPS = 5                 # cyclic Jacobi sweeps, each (0,1), (0,2), (1,2)
QUANT = f32(8192.0)        # 2^13 quanta per metre
QCLAMP = f32(2.0 ** 29)    # a coordinate is clamped to +-2^29 quanta, so differences fit int32 and squares int64
MIN_MID_EIG = 1.0          # the middle eigenvalue must exceed one squared quantum


class Params:
    """The fields of tsdf_segment_params."""

    def __init__(self, K, H, W, near_m=0.0, far_m=6.0, small_radius_m=0.05, large_radius_m=0.5, don_thresh=0.1,
                 seg_radius_m=0.05, min_cluster=15, max_cluster=1000000, overlap=0.5, inset=2):
        self.K = np.asarray(K, f32).ravel()
        self.H, self.W = int(H), int(W)
        self.near_m, self.far_m = f32(near_m), f32(far_m)
        self.small_radius_m, self.large_radius_m = f32(small_radius_m), f32(large_radius_m)
        self.don_thresh, self.seg_radius_m = f32(don_thresh), f32(seg_radius_m)
        self.min_cluster, self.max_cluster = int(min_cluster), int(max_cluster)
        self.overlap, self.inset = f32(overlap), int(inset)


def from_ctypes(p):
    return Params(list(p.cam_K), p.im_height, p.im_width, p.near_m, p.far_m, p.small_radius_m, p.large_radius_m, p.don_thresh,
                  p.seg_radius_m, p.min_cluster, p.max_cluster, p.overlap, p.inset)


def radius_quanta(r):
    """rintf(r * 8192): the radius in quanta."""
    return int(np.rint(f32(r) * QUANT))


def points(depth, p):
    """(P int64 [H, W, 3] in quanta, valid bool [H, W]) of a depth frame."""
    d = np.asarray(depth, f32).reshape(p.H, p.W)
    with np.errstate(invalid="ignore"):
        valid = np.isfinite(d) & (p.near_m < d) & (d <= p.far_m)
    d = np.where(valid, d, f32(0))
    fx, cx, fy, cy = p.K[0], p.K[2], p.K[4], p.K[5]
    u = np.arange(p.W, dtype=f32)[None, :]
    v = np.arange(p.H, dtype=f32)[:, None]
    x = ((u - cx) / fx * d).astype(f32)
    y = ((v - cy) / fy * d).astype(f32)

    def quant(c):
        q = np.rint((c * QUANT).astype(f32))
        return np.minimum(np.maximum(q, -QCLAMP), QCLAMP).astype(np.int64)

    P = np.stack([quant(x), quant(y), quant(d + np.zeros_like(x))], axis=-1)
    P[~valid] = 0
    return P, valid


def steps(d, valid, focal, r, size):
    """Lattice step along one axis: max(1, ceil(clamp(floorf(focal * r / d), 1, size) / T)), int64 [H, W]."""
    dd = np.where(valid, d, f32(1))
    with np.errstate(over="ignore", divide="ignore"):
        h = np.floor(((f32(focal) * f32(r)).astype(f32) / dd).astype(f32))
    h = np.minimum(np.maximum(h, f32(1)), f32(size))
    return (h.astype(np.int64) + (T - 1)) // T


def moments(depth, p, r):
    """(n, S1 [.., 3], S2 [.., 6]) int64 of the counted taps at radius r; S2 order xx, xy, xz, yy, yz, zz."""
    P, valid = points(depth, p)
    d = np.asarray(depth, f32).reshape(p.H, p.W)
    H, W = p.H, p.W
    R2 = radius_quanta(r) ** 2
    sx = steps(d, valid, p.K[0], r, W)
    sy = steps(d, valid, p.K[4], r, H)
    uu0 = np.broadcast_to(np.arange(W, dtype=np.int64)[None, :], (H, W))
    vv0 = np.broadcast_to(np.arange(H, dtype=np.int64)[:, None], (H, W))
    n = np.zeros((H, W), np.int64)
    S1 = np.zeros((H, W, 3), np.int64)
    S2 = np.zeros((H, W, 6), np.int64)
    for j in range(-T, T + 1):
        vv = vv0 + j * sy
        okv = (vv >= 0) & (vv < H)
        vc = np.clip(vv, 0, H - 1)
        for i in range(-T, T + 1):
            uu = uu0 + i * sx
            ins = okv & (uu >= 0) & (uu < W)
            uc = np.clip(uu, 0, W - 1)
            D = P[vc, uc] - P
            dist2 = D[..., 0] * D[..., 0] + D[..., 1] * D[..., 1] + D[..., 2] * D[..., 2]
            cnt = ins & valid & valid[vc, uc] & (dist2 <= R2)
            D = D * cnt[..., None]
            n += cnt
            S1 += D
            S2[..., 0] += D[..., 0] * D[..., 0]
            S2[..., 1] += D[..., 0] * D[..., 1]
            S2[..., 2] += D[..., 0] * D[..., 2]
            S2[..., 3] += D[..., 1] * D[..., 1]
            S2[..., 4] += D[..., 1] * D[..., 2]
            S2[..., 5] += D[..., 2] * D[..., 2]
    return n, S1, S2, P, valid


def jacobi(a00, a01, a02, a11, a12, a22):
    """SWEEPS cyclic Jacobi sweeps in double on arrays of symmetric 3 x 3 matrices; returns (diagonal [3], V [3][3]) with V's
    columns the eigenvectors.  A rotation whose off-diagonal entry is exactly 0 is skipped."""
    A = [[a00, a01, a02], [a01, a11, a12], [a02, a12, a22]]
    A = [[np.array(x, f64) for x in row] for row in A]
    one, zero = np.ones_like(A[0][0]), np.zeros_like(A[0][0])
    V = [[one.copy() if i == j else zero.copy() for j in range(3)] for i in range(3)]
    with np.errstate(all="ignore"):
        for _ in range(SWEEPS):
            for (p, q, r) in ((0, 1, 2), (0, 2, 1), (1, 2, 0)):
                apq = A[p][q]
                go = apq != 0.0
                theta = (A[q][q] - A[p][p]) / (2.0 * apq)
                t = np.where(theta >= 0.0, 1.0, -1.0) / (np.abs(theta) + np.sqrt(theta * theta + 1.0))
                c = 1.0 / np.sqrt(t * t + 1.0)
                s = t * c
                app = A[p][p] - t * apq
                aqq = A[q][q] + t * apq
                arp = c * A[r][p] - s * A[r][q]
                arq = s * A[r][p] + c * A[r][q]
                A[p][p] = np.where(go, app, A[p][p])
                A[q][q] = np.where(go, aqq, A[q][q])
                A[p][q] = A[q][p] = np.where(go, 0.0, apq)
                A[r][p] = A[p][r] = np.where(go, arp, A[r][p])
                A[r][q] = A[q][r] = np.where(go, arq, A[r][q])
                for k in range(3):
                    vkp = c * V[k][p] - s * V[k][q]
                    vkq = s * V[k][p] + c * V[k][q]
                    V[k][p] = np.where(go, vkp, V[k][p])
                    V[k][q] = np.where(go, vkq, V[k][q])
    return [A[0][0], A[1][1], A[2][2]], V


def normals(depth, p, r):
    """(normal float64 [H, W, 3], exists bool [H, W]) at radius r."""
    n, S1, S2, P, valid = moments(depth, p, r)
    nn = np.where(n > 0, n, 1).astype(f64)
    m = [S1[..., a].astype(f64) / nn for a in range(3)]
    idx = {(0, 0): 0, (0, 1): 1, (0, 2): 2, (1, 1): 3, (1, 2): 4, (2, 2): 5}
    cov = {ab: S2[..., k].astype(f64) / nn - m[ab[0]] * m[ab[1]] for ab, k in idx.items()}
    lam, V = jacobi(cov[0, 0], cov[0, 1], cov[0, 2], cov[1, 1], cov[1, 2], cov[2, 2])
    l0, l1, l2 = lam
    k = np.zeros(n.shape, np.int64)
    lmin = l0.copy()
    k = np.where(l1 < lmin, 1, k)
    lmin = np.where(l1 < lmin, l1, lmin)
    k = np.where(l2 < lmin, 2, k)
    lo01, hi01 = np.where(l1 < l0, l1, l0), np.where(l1 < l0, l0, l1)
    mid = np.where(l2 < lo01, lo01, np.where(l2 < hi01, l2, hi01))
    exists = valid & (n >= 3) & (mid > MIN_MID_EIG)
    nv = [np.where(k == 0, V[a][0], np.where(k == 1, V[a][1], V[a][2])) for a in range(3)]
    dot = (nv[0] * P[..., 0].astype(f64) + nv[1] * P[..., 1].astype(f64)) + nv[2] * P[..., 2].astype(f64)
    flip = dot > 0.0
    N = np.stack([np.where(flip, -c, c) for c in nv], axis=-1)
    return N, exists


def don_values(depth, p):
    """(don float64 [H, W], 0 where a normal is missing; both bool [H, W]): the part that does not depend on don_thresh."""
    ns, es = normals(depth, p, p.small_radius_m)
    nl, el = normals(depth, p, p.large_radius_m)
    dv = ns - nl
    val = 0.5 * np.sqrt((dv[..., 0] * dv[..., 0] + dv[..., 1] * dv[..., 1]) + dv[..., 2] * dv[..., 2])
    both = es & el
    return np.where(both, val, 0.0), both


def don(depth, p, values=None):
    """(don float32 [H, W], kept bool [H, W]); values: don_values(depth, p) when the caller has it already."""
    val, both = don_values(depth, p) if values is None else values
    kept = both & (val > f64(p.don_thresh))
    return val.astype(f32), kept


def clusters_of(kept, P, p):
    """(cluster int32 [H, W], C) of a kept image and its points."""
    H, W = kept.shape
    Rs2 = radius_quanta(p.seg_radius_m) ** 2
    flat = np.arange(H * W, dtype=np.int64).reshape(H, W)

    def joined(a, b, Pa, Pb):
        D = Pa - Pb
        return a & b & ((D * D).sum(axis=-1) <= Rs2)

    eh = joined(kept[:, :-1], kept[:, 1:], P[:, :-1], P[:, 1:])
    ev = joined(kept[:-1, :], kept[1:, :], P[:-1, :], P[1:, :])
    ea = np.concatenate([flat[:, :-1][eh], flat[:-1, :][ev]]).tolist()
    eb = np.concatenate([flat[:, 1:][eh], flat[1:, :][ev]]).tolist()
    parent = list(range(H * W))

    def find(a):
        r = a
        while parent[r] != r:
            r = parent[r]
        while parent[a] != r:
            parent[a], a = r, parent[a]
        return r

    for a, b in zip(ea, eb):
        ra, rb = find(a), find(b)
        if ra < rb:
            parent[rb] = ra
        elif rb < ra:
            parent[ra] = rb
    kidx = np.nonzero(kept.ravel())[0]
    root = np.full(H * W, -1, np.int64)
    root[kidx] = [find(int(a)) for a in kidx]
    size = np.bincount(root[kidx], minlength=H * W) if kidx.size else np.zeros(H * W, np.int64)
    ok_root = (size >= p.min_cluster) & (size <= p.max_cluster) & (size > 0)
    number = np.cumsum(ok_root) * ok_root                     # 1..C in the order of the roots = smallest flat index
    out = np.zeros(H * W, np.int32)
    out[kidx] = number[root[kidx]]
    return out.reshape(H, W), int(ok_root.sum())


def segment_depth(depth, p, values=None):
    """(don float32 [H, W], cluster int32 [H, W], C); values: see don."""
    dn, kept = don(depth, p, values)
    P, _ = points(depth, p)
    cl, C = clusters_of(kept, P, p)
    return dn, cl, C


def deep(masks, inset):
    """deep [K, H, W]: every pixel of the (2 inset + 1)^2 square is in the mask; outside the image counts as not in."""
    inn = np.asarray(masks, np.uint8) >= 128
    K, H, W = inn.shape
    pad = np.zeros((K, H + 2 * inset, W + 2 * inset), bool)
    pad[:, inset:inset + H, inset:inset + W] = inn
    out = np.ones((K, H, W), bool)
    for dy in range(2 * inset + 1):
        for dx in range(2 * inset + 1):
            out &= pad[:, dy:dy + H, dx:dx + W]
    return out


def refine(cluster, C, masks, p):
    """(out uint8 [K, H, W], counts uint32 [C + C K]: size[c] then inside[c][k]) -- labels outside 1..C count as none."""
    masks = np.asarray(masks, np.uint8)
    K = masks.shape[0]
    cl = np.asarray(cluster, np.int64).reshape(masks.shape[1:])
    lab = (cl >= 1) & (cl <= C)
    c0 = np.where(lab, cl - 1, 0)
    dp = deep(masks, p.inset)
    size = np.bincount(c0[lab], minlength=C).astype(np.int64)
    inside = np.zeros((C, K), np.int64)
    for k in range(K):
        inside[:, k] = np.bincount(c0[lab & dp[k]], minlength=C)
    with np.errstate(invalid="ignore", divide="ignore"):
        accept = (inside.astype(np.uint32).astype(f32) / size.astype(np.uint32).astype(f32)[:, None]) > p.overlap
    out = np.zeros(masks.shape, np.uint8)
    for k in range(K if C else 0):
        out[k][lab & dp[k] & accept[c0, k]] = 255
    counts = np.concatenate([size, inside.ravel()]).astype(np.uint32)
    return out, counts


def segment_frame(depth, masks, p):
    """(out uint8 [K, H, W], cluster int32 [H, W], C)."""
    _, cl, C = segment_depth(depth, p)
    out, _ = refine(cl, C, masks, p)
    return out, cl, C
