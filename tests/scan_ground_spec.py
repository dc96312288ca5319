"""The ground rule of csrc/tsdf_scan_ground.hip.h restated in float32 NumPy (test infrastructure, no GPU): the cell of a point
in the n_rings x n_columns spherical image (ref: src/Utility.cpp:452-496), "a later point overwrites an earlier one", the state
of a cell from the step to the cell one ring above it (ref: :498-553) and the flag of a point.  Every operation is one float32
operation in the written order.  The device finds a point's ring and column by bisection; here both are LINEAR COUNTS over the
whole table or run, and `mark` asserts on the way that the tests are monotone along what is counted, which is what makes the two
the same (csrc/scan_ground_tables.h has the argument).  The tables come from the library's own host-only builder
(capi.scan_ground_tables), so that the restatement is held to the rule and not to a second libm; `tables_numpy` builds them a
second time in NumPy for the tests that compare the two.  `mark_scalar` states the rule once more, point by point and cell by
cell, with nothing vectorised."""
import collections

import numpy as np

from semantic_slam_amd import capi

F = np.float32
FLT_MAX = np.finfo(np.float32).max
NO_CELL = -1
DROP_GROUND, ONLY_GROUND = 0, 1

Params = collections.namedtuple("Params", "n_rings n_columns ang_res_y ang_bottom mount_deg tol_deg min_range ground_rings mark_upper")
# the reference's literals (ref: include/Utility.hpp:52-58, src/Utility.cpp:484,529): they cover -15.1 ... +11.8 degrees
DEFAULT = Params(64, 4500, F(26.9) / F(63.0), F(15.1), F(0.0), F(2.5), F(0.1), 63, 0)
# an HDL-64E fires +2 ... -24.8 degrees; each beam at its ring's centre
_RES = F(26.8) / F(63.0)
HDL64E = DEFAULT._replace(ang_res_y=_RES, ang_bottom=F(24.8) + _RES / F(2.0))


def params(p=None, **kw):
    """A Params from None (the defaults), a Params or a capi.ScanGroundParams, with fields replaced."""
    if p is None:
        p = DEFAULT
    elif isinstance(p, capi.ScanGroundParams):
        p = Params(*(getattr(p, f) for f in Params._fields))
    p = p._replace(**kw)
    return p._replace(ang_res_y=F(p.ang_res_y), ang_bottom=F(p.ang_bottom), mount_deg=F(p.mount_deg), tol_deg=F(p.tol_deg),
                      min_range=F(p.min_range))


def to_capi(p):
    return capi.ScanGroundParams(int(p.n_rings), int(p.n_columns), float(p.ang_res_y), float(p.ang_bottom), float(p.mount_deg),
                                 float(p.tol_deg), float(p.min_range), int(p.ground_rings), int(p.mark_upper))


def tables(p):
    """The library's tables of p (host arithmetic only)."""
    return capi.scan_ground_tables(to_capi(p))


def quadrant(a, b):
    """0: a > 0 && b >= 0, 1: a <= 0 && b > 0, 2: a < 0 && b <= 0, 3: a >= 0 && b < 0; -1 for (0, 0) and NaN.  Arrays or scalars."""
    a, b = np.asarray(a, F), np.asarray(b, F)
    q = np.full(np.broadcast(a, b).shape, -1, np.int64)
    q = np.where((a > 0) & (b >= 0), 0, q)
    q = np.where((a <= 0) & (b > 0), 1, q)
    q = np.where((a < 0) & (b <= 0), 2, q)
    q = np.where((a >= 0) & (b < 0), 3, q)
    return q


def tables_numpy(p):
    """The same tables from NumPy's libm, in double and rounded once, and the quadrants' runs found by walking the columns."""
    r = np.arange(p.n_rings + 1, dtype=np.float64)
    T = np.tan(np.deg2rad(r * np.float64(p.ang_res_y) - np.float64(p.ang_bottom))).astype(F)
    c = np.arange(p.n_columns, dtype=np.float64)
    beta = np.deg2rad((c - float(p.n_columns // 2) - 0.5) * 360.0 / p.n_columns)
    Cc, S = np.cos(beta).astype(F), np.sin(beta).astype(F)
    tlo = F(np.tan(np.deg2rad(np.float64(p.mount_deg) - np.float64(p.tol_deg))))
    thi = F(np.tan(np.deg2rad(np.float64(p.mount_deg) + np.float64(p.tol_deg))))
    q = quadrant(Cc, S)
    first, length = np.zeros(4, np.int32), np.zeros(4, np.int32)
    for k in range(4):
        length[k] = np.count_nonzero(q == k)
        starts = [i for i in range(p.n_columns) if q[i] == k and q[i - 1] != k]
        assert len(starts) == 1, (k, starts)
        first[k] = starts[0]
    return {"T": T, "C": Cc, "S": S, "tlo": tlo, "thi": thi, "first": first, "len": length}


def _monotone(pred):
    """True where a row of tests is true up to some position and false behind it."""
    return np.all(pred[:, :-1] | ~pred[:, 1:], axis=1) if pred.shape[1] > 1 else np.ones(len(pred), bool)


def cells(points, p, tab, chunk=4096):
    """Per point: {"ring", "col": -1 where the point has no cell, "cell": ring * n_columns + col or NO_CELL, "k": the count in the
    column's run (-1 without a cell), "range": float32, "why": 0 a cell, 1 not finite, 2 h not > 0, 3 below min_range, 4 ring
    below 0, 5 ring at or above n_rings}."""
    pts = np.asarray(points, F).reshape(-1, 4)
    n = len(pts)
    x, y, z = pts[:, 0], pts[:, 1], pts[:, 2]
    T, Cc, S = tab["T"], tab["C"], tab["S"]
    with np.errstate(all="ignore"):
        hh = x * x + y * y
        h = np.sqrt(hh)
        rng = np.sqrt(hh + z * z)
        assert h.dtype == F and rng.dtype == F
        finite = np.isfinite(x) & np.isfinite(y) & np.isfinite(z)
        pred = z[:, None] >= T[None, :] * h[:, None]
        assert np.all(_monotone(pred)[finite]), "the ring test is not monotone"
        ring = np.count_nonzero(pred, axis=1) - 1
    why = np.where(~finite, 1, np.where(~(h > F(0)), 2, np.where(~(rng >= F(p.min_range)), 3,
                   np.where(ring < 0, 4, np.where(ring >= p.n_rings, 5, 0))))).astype(np.int32)
    ok = why == 0
    col = np.full(n, -1, np.int64)
    k_of = np.full(n, -1, np.int64)
    q = quadrant(x, y)
    for quad in range(4):
        idx = np.flatnonzero(ok & (q == quad))
        run = (int(tab["first"][quad]) + np.arange(int(tab["len"][quad]))) % p.n_columns
        for s in range(0, len(idx), chunk):
            i = idx[s:s + chunk]
            with np.errstate(all="ignore"):
                pr = Cc[run][None, :] * y[i][:, None] >= S[run][None, :] * x[i][:, None]      # two products compared
            assert np.all(_monotone(pr)), "the column test is not monotone"
            k = np.count_nonzero(pr, axis=1)
            k_of[i] = k
            col[i] = (int(tab["first"][quad]) + k - 1) % p.n_columns
    assert np.all(col[ok] >= 0)
    ring = np.where(ok, ring, -1)
    return {"ring": ring, "col": col, "cell": np.where(ok, ring * p.n_columns + col, NO_CELL), "k": k_of, "range": rng, "why": why}


def pair_states(pts, winner, p, tab):
    """[n_rings - 1, n_columns] int8: the pair of cells (r, c), (r + 1, c): -1 one of them empty, 1 level, 0 not."""
    lo, hi = winner[:-1], winner[1:]
    both = (lo >= 0) & (hi >= 0)
    if len(pts) == 0:
        return np.full(lo.shape, -1, np.int8)
    a, b = pts[np.where(both, lo, 0)], pts[np.where(both, hi, 0)]
    with np.errstate(all="ignore"):
        dx, dy, dz = b[..., 0] - a[..., 0], b[..., 1] - a[..., 1], b[..., 2] - a[..., 2]
        hd = np.sqrt(dx * dx + dy * dy)
        assert hd.dtype == F
        level = (dz >= F(tab["tlo"]) * hd) & (dz <= F(tab["thi"]) * hd)
    return np.where(both, level.astype(np.int8), np.int8(-1)).astype(np.int8)


def mark(points, p, tab=None):
    """The whole rule: {"flags": [n] uint8, "state": [n_rings, n_columns] int8, "winner": [n_rings, n_columns] int32, "counts": [4]
    int64 (points with a cell, occupied cells, ground cells, ground points), "cells": what `cells` returns}."""
    tab = tables(p) if tab is None else tab
    pts = np.ascontiguousarray(points, F).reshape(-1, 4)
    c = cells(pts, p, tab)
    has = c["cell"] != NO_CELL
    winner = np.full(p.n_rings * p.n_columns, -1, np.int64)
    np.maximum.at(winner, c["cell"][has], np.flatnonzero(has))          # the serial loop's result: the highest index stays
    winner = winner.reshape(p.n_rings, p.n_columns)
    pair = pair_states(pts, winner, p, tab)
    looked = np.arange(p.n_rings - 1)[:, None] < p.ground_rings             # pairs r < ground_rings are looked at
    own = np.zeros((p.n_rings, p.n_columns), np.int8)
    own[:-1] = np.where(looked, pair, 0)
    below = np.zeros((p.n_rings, p.n_columns), bool)
    if p.mark_upper:
        below[1:] = looked & (pair == 1)
    state = np.where(own < 0, -1, np.where((own == 1) | below, 1, 0)).astype(np.int8)
    flags = np.full(len(pts), 2, np.uint8)
    flags[has] = (state.ravel()[c["cell"][has]] == 1).astype(np.uint8)
    counts = np.array([np.count_nonzero(has), np.count_nonzero(winner >= 0), np.count_nonzero(state == 1), np.count_nonzero(flags == 1)],
                      np.int64)
    return {"flags": flags, "state": state, "winner": winner.astype(np.int32), "counts": counts, "cells": c}


def mark_scalar(points, p, tab=None):
    """`mark` once more with nothing vectorised: a loop over the points, then a loop over the cells; linear counts.  The same
    four results."""
    tab = tables(p) if tab is None else tab
    T, Cc, S = [F(v) for v in tab["T"]], [F(v) for v in tab["C"]], [F(v) for v in tab["S"]]
    tlo, thi = F(tab["tlo"]), F(tab["thi"])
    pts = np.ascontiguousarray(points, F).reshape(-1, 4)
    nr, nc = p.n_rings, p.n_columns
    cell_of = []
    winner = [[-1] * nc for _ in range(nr)]
    with np.errstate(all="ignore"):
        for i, (x, y, z, _) in enumerate(pts):
            hh = F(F(x * x) + F(y * y))
            h, rng = np.sqrt(hh), np.sqrt(F(hh + F(z * z)))
            cell = None
            if np.isfinite(x) and np.isfinite(y) and np.isfinite(z) and h > 0 and rng >= F(p.min_range):
                ring = sum(1 for r in range(nr + 1) if z >= F(T[r] * h)) - 1
                if 0 <= ring < nr:
                    quad = 0 if (x > 0 and y >= 0) else 1 if (x <= 0 and y > 0) else 2 if (x < 0 and y <= 0) else 3
                    first, length = int(tab["first"][quad]), int(tab["len"][quad])
                    k = sum(1 for j in range(length) if F(Cc[(first + j) % nc] * y) >= F(S[(first + j) % nc] * x))
                    cell = (ring, (first + k - 1) % nc)
                    winner[ring][cell[1]] = i                         # in serial order: a later point overwrites
            cell_of.append(cell)

        def pair(r, c):
            lo, hi = winner[r][c], winner[r + 1][c]
            if lo < 0 or hi < 0:
                return -1
            dx, dy, dz = F(pts[hi, 0] - pts[lo, 0]), F(pts[hi, 1] - pts[lo, 1]), F(pts[hi, 2] - pts[lo, 2])
            hd = np.sqrt(F(F(dx * dx) + F(dy * dy)))
            return 1 if (dz >= F(tlo * hd) and dz <= F(thi * hd)) else 0

        state = np.zeros((nr, nc), np.int8)
        for r in range(nr):
            for c in range(nc):
                own = pair(r, c) if r < p.ground_rings else 0
                below = pair(r - 1, c) if (p.mark_upper and r >= 1 and r - 1 < p.ground_rings) else 0
                state[r, c] = -1 if own < 0 else 1 if (own == 1 or below == 1) else 0
    flags = np.array([2 if c is None else int(state[c] == 1) for c in cell_of], np.uint8).reshape(-1)
    win = np.array(winner, np.int32).reshape(nr, nc)
    counts = np.array([sum(c is not None for c in cell_of), np.count_nonzero(win >= 0), np.count_nonzero(state == 1),
                       np.count_nonzero(flags == 1)], np.int64)
    return {"flags": flags, "state": state, "winner": win, "counts": counts}


def select(points, flags, which):
    """The points that DROP_GROUND (flag != 1) or ONLY_GROUND (flag == 1) keeps, in their order."""
    pts = np.asarray(points, F).reshape(-1, 4)
    keep = (flags == 1) if which == ONLY_GROUND else (flags != 1)
    return np.ascontiguousarray(pts[keep])


# ---- the reference's own formula, in float64 (ref: src/Utility.cpp:469-481): what the rule above is a restatement OF --------
def reference_cells(points, p):
    """(ring coordinate, column coordinate, ring, column) per point by atan2 in float64: ring = trunc((elevation + ang_bottom) /
    ang_res_y), column = -round((atan2(x, y) deg - 90) / res_x) + n_columns / 2, wrapped once.  The coordinates say how far a
    point is from a cell's border: the ring's is at its integers, the column's at its half-integers."""
    pts = np.asarray(points, np.float64).reshape(-1, 4)
    x, y, z = pts[:, 0], pts[:, 1], pts[:, 2]
    ring_f = (np.degrees(np.arctan2(z, np.sqrt(x * x + y * y))) + np.float64(p.ang_bottom)) / np.float64(p.ang_res_y)
    res_x = 360.0 / p.n_columns
    col_f = -(np.degrees(np.arctan2(x, y)) - 90.0) / res_x + p.n_columns // 2
    ring = np.floor(ring_f).astype(np.int64)
    col = np.floor(col_f + 0.5).astype(np.int64)
    col = np.where(col >= p.n_columns, col - p.n_columns, col)
    return ring_f, col_f, ring, col
