"""The lidar rule of csrc/tsdf_scan.hip.h restated in float32 NumPy (test infrastructure, no GPU): the projection of a scan
to a range image with the reference's serial "a later point overwrites an earlier one" (ref: src/Utility.cpp:40-57,
401-413), range to z-depth (ref: src/Object.cpp:613-620, src/DoN.cpp:89-96) and the composition of velo2img (ref:
src/Utility.cpp:42-49).  Every operation is one float32 operation in the written order, so the device, built with contraction
off and correctly rounded division and square root, must give the same bits.  OpenCV is absent, so the reference's own
functions cannot be compiled: this restatement of the cited lines is what the library is held to."""
import numpy as np

F = np.float32
FLT_MAX = np.finfo(np.float32).max
MAX_POINTS = 0xFFFFFFFF          # a point's index + 1 is the upper word of its pixel's key

# why a point is not written
ACCEPTED, BELOW_GUARD, OUTSIDE, NO_RANGE = 0, 1, 2, 3


def compose(P_rect, R_rect, R_velo, t_velo):
    """velo2img [3, 4] = P_rect * [R_rect 0; 0 1] * [R_velo t_velo; 0 1], each entry the left-to-right sum
    ((a0 b0 + a1 b1) + a2 b2) + a3 b3 in float32, as tsdf_multiply_matrix forms it."""
    P = np.zeros((4, 4), F)
    P[:3] = np.asarray(P_rect, F).reshape(3, 4)
    A, B = np.eye(4, dtype=F), np.eye(4, dtype=F)
    A[:3, :3] = np.asarray(R_rect, F).reshape(3, 3)
    B[:3, :3] = np.asarray(R_velo, F).reshape(3, 3)
    B[:3, 3] = np.asarray(t_velo, F).reshape(3)

    def mul(a, b):
        out = np.zeros((4, 4), F)
        for i in range(4):
            for j in range(4):
                acc = F(a[i, 0] * b[0, j])
                for k in range(1, 4):
                    acc = F(acc + F(a[i, k] * b[k, j]))
                out[i, j] = acc
        return out

    with np.errstate(all="ignore"):
        return mul(mul(P, A), B)[:3].copy()


def project_full(points, velo2img, H, W):
    """The projection with everything the cases ask about: {"range": image [H, W], "n_pixels", "reason": per point one of
    ACCEPTED / BELOW_GUARD / OUTSIDE / NO_RANGE, "h2": per point, "u", "v": per point (-1 unless accepted), "winner": per
    pixel the index of the point that stays, -1 where none}."""
    pts = np.asarray(points, F).reshape(-1, 4)
    M = np.asarray(velo2img, F).reshape(3, 4)
    n = len(pts)
    assert n <= MAX_POINTS
    x, y, z = pts[:, 0], pts[:, 1], pts[:, 2]
    with np.errstate(all="ignore"):
        h = [((M[k, 0] * x + M[k, 1] * y) + M[k, 2] * z) + M[k, 3] for k in range(3)]
        assert all(a.dtype == F for a in h)
        guard = h[0] >= F(2)                                              # ref: src/Utility.cpp:53
        uf, vf = h[0] / h[2], h[1] / h[2]
        inside = (uf >= F(1)) & (uf < F(W)) & (vf >= F(1)) & (vf < F(H))  # float comparisons in front of the cast
        rng = np.sqrt((x * x + y * y) + z * z)
        assert rng.dtype == F
        has_range = rng > F(0)
    reason = np.where(~guard, BELOW_GUARD, np.where(~inside, OUTSIDE, np.where(~has_range, NO_RANGE, ACCEPTED))).astype(np.int32)
    acc = np.flatnonzero(reason == ACCEPTED)
    u = np.full(n, -1, np.int64)
    v = np.full(n, -1, np.int64)
    u[acc] = uf[acc].astype(np.int32)           # truncation, of values in [1, W) only
    v[acc] = vf[acc].astype(np.int32)
    # the serial loop's result: per pixel the accepted point with the highest index
    winner = np.full(H * W, -1, np.int64)
    np.maximum.at(winner, v[acc] * W + u[acc], acc)
    image = np.zeros(H * W, F)
    image[winner >= 0] = rng[winner[winner >= 0]]
    return {"range": image.reshape(H, W), "n_pixels": int(np.count_nonzero(winner >= 0)), "reason": reason, "h2": h[2],
            "u": u, "v": v, "winner": winner.reshape(H, W)}


def project(points, velo2img, H, W):
    """(range image [H, W] float32, number of written pixels)."""
    r = project_full(points, velo2img, H, W)
    return r["range"], r["n_pixels"]


def range_to_depth(range_im, K):
    """z-depth [H, W] of a range image under K (9 floats, row-major): range / sqrtf((x x + y y) + 1) where 0 < range <=
    FLT_MAX, else 0."""
    r = np.asarray(range_im, F)
    H, W = r.shape
    K = np.asarray(K, F).reshape(9)
    fx, fy, cx, cy = K[0], K[4], K[2], K[5]
    with np.errstate(all="ignore"):
        x = (np.arange(W, dtype=F) - cx) / fx
        y = (np.arange(H, dtype=F) - cy) / fy
        rim = np.sqrt((x[None, :] * x[None, :] + y[:, None] * y[:, None]) + F(1))
        assert rim.dtype == F
        d = np.where((r > F(0)) & (r <= FLT_MAX), r / rim, F(0))
    return np.ascontiguousarray(d, F)


def scan_depth(points, velo2img, K, H, W):
    """The z-depth image of a scan: what tsdf_integrate_scan fuses."""
    return range_to_depth(project(points, velo2img, H, W)[0], K)
