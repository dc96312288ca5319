"""NumPy restatement of the association rule: the per-pixel counts of csrc/tsdf_associate.hip.h and the host assignment of
include/tsdf_hip.h (tsdf_associate_count / tsdf_associate_assign / tsdf_batch_associate).

Per-pixel tests are float32 in the order the kernel evaluates them, so `counts` equals the device's block word for word; the
assignment is integer and float64 arithmetic as the host does it, with exact (Python integer) IoU comparisons."""
import numpy as np

f32 = np.float32
AGREE, FRONT, BEHIND, LIVE_INVALID = 0, 1, 2, 3


class Params:
    """The fields of tsdf_associate_params the rule reads."""

    def __init__(self, near_m=0.0, far_m=6.0, depth_tol_m=0.02, min_pixels=25, min_iou=0.25, one_to_one=1):
        self.near_m, self.far_m, self.depth_tol_m = f32(near_m), f32(far_m), f32(depth_tol_m)
        self.min_pixels, self.min_iou, self.one_to_one = int(min_pixels), f32(min_iou), int(one_to_one)


def from_ctypes(p):
    return Params(p.ray.near_m, p.ray.far_m, p.depth_tol_m, p.min_pixels, p.min_iou, p.one_to_one)


def n_words(k, m):
    return 3 * k * m + 3 * k + 4 * m


def split(block, k, m):
    """overlap [k, m, 3], mask [k, 3], member [m, 4] views of a block."""
    n_ov = 3 * k * m
    return block[:n_ov].reshape(k, m, 3), block[n_ov:n_ov + 3 * k].reshape(k, 3), block[n_ov + 3 * k:].reshape(m, 4)


def classes(member, rdepth, depth, n_members, p):
    """Per pixel: (rendered, live valid, class) with class 0..3 for rendered pixels (agree, front, behind, live invalid)."""
    member = np.asarray(member, np.int32).ravel()
    rd = np.asarray(rdepth, f32).ravel()
    d = np.asarray(depth, f32).ravel()
    with np.errstate(invalid="ignore"):
        valid = np.isfinite(d) & (p.near_m < d) & (d <= p.far_m)
        rendered = (member >= 0) & (member < n_members)
        r = (d - rd).astype(f32)
        tol = f32(p.depth_tol_m)
        cls = np.where(np.abs(r) <= tol, AGREE, np.where(r < -tol, FRONT, BEHIND))
    cls = np.where(valid, cls, LIVE_INVALID)
    return rendered, valid, cls


def counts(member, rdepth, depth, masks, n_members, p):
    """The count block (uint32, 3KM + 3K + 4M words) of images member [H, W] int32, rdepth / depth [H, W] float32 and masks
    [K, H, W] uint8."""
    masks = np.asarray(masks, np.uint8)
    K = masks.shape[0]
    M = int(n_members)
    rendered, valid, cls = classes(member, rdepth, depth, M, p)
    mem = np.asarray(member, np.int64).ravel()
    inm = masks.reshape(K, -1) >= 128
    out = np.zeros(n_words(K, M), np.uint64)
    ov, mk, mb = split(out, K, M)
    mb[:] = np.bincount(np.where(rendered, mem * 4 + cls, 4 * M), minlength=4 * M + 1)[:4 * M].reshape(M, 4)
    for k in range(K):
        s = inm[k]
        mk[k] = (s.sum(), (s & valid).sum(), (s & valid & ~rendered).sum())
        sel = s & rendered & (cls < 3)
        ov[k] = np.bincount(mem[sel] * 3 + cls[sel], minlength=3 * M).reshape(M, 3)
    return out.astype(np.uint32)


def assign(block, k, n_members, p, labels=None):
    """(assign int32 [k], iou float32 [k]) of a count block; labels None or (mask_label, mask_score, member_label,
    member_score).  A block with overlap[k][m][agree] above mask[k][1] or member[m][0] is refused (ValueError)."""
    ov, mk, mb = split(np.asarray(block, np.uint32), k, n_members)
    a_all = ov[:, :, AGREE].astype(np.int64)
    if (a_all > mk[:, 1:2].astype(np.int64)).any() or (a_all > mb[None, :, 0].astype(np.int64)).any():
        raise ValueError("inconsistent counts")
    cand = []
    for i in range(k):
        for m in range(n_members):
            a = int(ov[i, m, AGREE])
            u = int(mk[i, 1]) + int(mb[m, 0]) - a
            if a < p.min_pixels or not (float(a) >= float(p.min_iou) * float(u)):
                continue
            if labels is not None:
                ml, ms, bl, bs = labels
                if not (int(ml[i]) == int(bl[m]) or f32(bs[m]) > f32(f32(1.1) * f32(ms[i]))):
                    continue
            cand.append((i, m, a, u))
    pick = [None] * k
    if p.one_to_one:
        # descending a / u exactly; equal IoUs keep (k, m) order (a stable sort on the exact fraction)
        from fractions import Fraction
        order = sorted(cand, key=lambda c: (-Fraction(c[2], c[3]), c[0], c[1]))
        used_m = set()
        for c in order:
            if pick[c[0]] is None and c[1] not in used_m:
                pick[c[0]] = c
                used_m.add(c[1])
    else:
        for c in cand:
            b = pick[c[0]]
            if b is None or c[2] * b[3] > b[2] * c[3]:
                pick[c[0]] = c
    out = np.full(k, -1, np.int32)
    iou = np.zeros(k, f32)
    for i, c in enumerate(pick):
        if c is not None:
            out[i] = c[1]
            iou[i] = f32(float(c[2]) / float(c[3]))
    return out, iou
