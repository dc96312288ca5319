"""The fill rule of csrc/tsdf_scan_fill.hip.h restated in float32 NumPy (test infrastructure, no GPU): a sparse
z-depth image is made denser by interpolating INVERSE depth between the nearest measured pixels on either side, along rows
first (the u pass) and then along columns (the v pass, which reads the u pass's output).  Every operation is one float32
operation in the written order, so the device, built with contraction off, correctly rounded division and denormals kept,
must give the same bits.  fill() is the vectorised restatement the library is held to; fill_scalar() states the same rule a
second time, pixel by pixel, and tests/test_scan_fill_spec.py holds the two to each other."""
import numpy as np

F = np.float32
FLT_MAX = np.finfo(np.float32).max
MAX_SPAN = 16
DEFAULT = (5, 8, F(0.05))            # tsdf_scan_fill_params_default: max_span_u, max_span_v, jump_rel
EMPTY, MEASURED, FILLED_U, FILLED_V = 0, 1, 2, 3


def params_ok(max_span_u, max_span_v, jump_rel):
    """What the library accepts: spans in 0 ... 16, jump_rel finite and >= 0."""
    j = F(jump_rel)
    return 0 <= int(max_span_u) <= MAX_SPAN and 0 <= int(max_span_v) <= MAX_SPAN and bool(np.isfinite(j)) and bool(j >= 0)


def is_source(x):
    x = np.asarray(x, F)
    with np.errstate(all="ignore"):
        return (x > F(0)) & (x <= FLT_MAX)


def fill_line_pass(x, max_span, jump_rel):
    """One pass along the LAST axis of x [n, len]: (output, filled mask).  A pixel that is not filled keeps its input bits."""
    x = np.ascontiguousarray(x, F)
    out = x.copy()
    n, length = x.shape
    filled = np.zeros(x.shape, bool)
    if max_span <= 1:
        return out, filled
    src = is_source(x)
    da = np.zeros(x.shape, np.int32)
    db = np.zeros(x.shape, np.int32)
    a = np.zeros(x.shape, F)
    b = np.zeros(x.shape, F)
    for k in range(1, min(int(max_span), length)):        # distances 1 ... max_span - 1, inside the line
        take = np.zeros(x.shape, bool)
        take[:, k:] = src[:, :-k]
        take &= da == 0
        da[take] = k
        a[:, k:][take[:, k:]] = x[:, :-k][take[:, k:]]
        take = np.zeros(x.shape, bool)
        take[:, :-k] = src[:, k:]
        take &= db == 0
        db[take] = k
        b[:, :-k][take[:, :-k]] = x[:, k:][take[:, :-k]]
    pair = ~src & (da > 0) & (db > 0) & (da + db <= int(max_span))
    with np.errstate(all="ignore"):
        a1, b1 = np.where(pair, a, F(1)), np.where(pair, b, F(1))
        near = np.abs(a1 - b1) <= F(jump_rel) * np.minimum(a1, b1)
        ia = F(1) / a1
        ib = F(1) / b1
        num = ia * db.astype(F) + ib * da.astype(F)
        inv = num / (da + db).astype(F)
        d = F(1) / inv
        assert all(t.dtype == F for t in (a1, b1, ia, ib, num, inv, d))
        filled = pair & near & (d > F(0)) & (d <= FLT_MAX)
    out[filled] = d[filled]
    return out, filled


def fill(depth, max_span_u=DEFAULT[0], max_span_v=DEFAULT[1], jump_rel=DEFAULT[2]):
    """(filled image [H, W] float32, kind [H, W] uint8, n_filled) of a sparse z-depth image."""
    assert params_ok(max_span_u, max_span_v, jump_rel)
    x = np.ascontiguousarray(depth, F)
    assert x.ndim == 2
    measured = is_source(x)
    after_u, by_u = fill_line_pass(x, int(max_span_u), F(jump_rel))
    after_v_t, by_v_t = fill_line_pass(np.ascontiguousarray(after_u.T), int(max_span_v), F(jump_rel))
    out, by_v = np.ascontiguousarray(after_v_t.T), by_v_t.T
    assert not np.any(by_u & measured) and not np.any(by_v & (measured | by_u))
    kind = np.zeros(x.shape, np.uint8)
    kind[measured] = MEASURED
    kind[by_u] = FILLED_U
    kind[by_v] = FILLED_V
    return out, kind, int(np.count_nonzero(by_u) + np.count_nonzero(by_v))


# ---- the same rule, one pixel at a time -----------------------------------------------------------------------------
def _scalar_source(d):
    return bool(d > F(0)) and bool(d <= FLT_MAX)


def _scalar_line(line, i, max_span, jump_rel):
    """The value of pixel i of a line after one pass, and whether the pass filled it."""
    x = line[i]
    if _scalar_source(x) or max_span <= 1:
        return x, False
    da = db = 0
    for k in range(1, max_span):
        if i - k >= 0 and _scalar_source(line[i - k]):
            da = k
            break
    for k in range(1, max_span):
        if i + k < len(line) and _scalar_source(line[i + k]):
            db = k
            break
    if da == 0 or db == 0 or da + db > max_span:
        return x, False
    a, b = F(line[i - da]), F(line[i + db])
    with np.errstate(all="ignore"):
        if not bool(F(abs(F(a - b))) <= F(F(jump_rel) * min(a, b))):
            return x, False
        ia = F(F(1) / a)
        ib = F(F(1) / b)
        num = F(F(ia * F(db)) + F(ib * F(da)))
        inv = F(num / F(da + db))
        d = F(F(1) / inv)
    if _scalar_source(d):
        return d, True
    return x, False


def fill_scalar(depth, max_span_u=DEFAULT[0], max_span_v=DEFAULT[1], jump_rel=DEFAULT[2], rows=None):
    """fill() stated pixel by pixel; rows = (first, last + 1) restricts the OUTPUT to those rows (read from the whole image)."""
    x = np.ascontiguousarray(depth, F)
    H, W = x.shape
    r0, r1 = (0, H) if rows is None else rows
    lo, hi = max(0, r0 - MAX_SPAN), min(H, r1 + MAX_SPAN)
    after_u = x.copy()
    kind = np.zeros(x.shape, np.uint8)
    for v in range(lo, hi):
        for u in range(W):
            if _scalar_source(x[v, u]):
                kind[v, u] = MEASURED
                continue
            after_u[v, u], f = _scalar_line(x[v], u, int(max_span_u), jump_rel)
            if f:
                kind[v, u] = FILLED_U
    out = after_u.copy()
    for u in range(W):
        col = after_u[lo:hi, u]
        for v in range(r0, r1):
            if kind[v, u] != EMPTY:
                continue
            out[v, u], f = _scalar_line(col, v - lo, int(max_span_v), jump_rel)
            if f:
                kind[v, u] = FILLED_V
    n = int(np.count_nonzero(kind[r0:r1] >= FILLED_U))
    return out[r0:r1], kind[r0:r1], n
