"""The named ground cases (test infrastructure, no GPU): the smallest inputs at which the kernels of csrc/tsdf_scan_ground.hip.h
can go wrong.  Each case is built once, asserts here, on the CPU, that the restatement (tests/scan_ground_spec.py) reaches the
branch it is named for, and carries the restatement's results; tests/test_scan_ground_spec.py runs the assertions and the second,
scalar statement over them, tests/test_gpu_scan_ground.py holds the device to the results bit for bit."""
import functools

import numpy as np

import scan_cases
import scan_fill_spec
import scan_ground_spec as spec
import scan_spec
from semantic_slam_amd import synth

F = np.float32
up = lambda a: np.nextafter(F(a), F(np.inf))          # noqa: E731
down = lambda a: np.nextafter(F(a), F(-np.inf))       # noqa: E731

# 5 rings of 10 degrees from -25, 36 columns of 10 degrees (their borders at the odd multiples of 5 degrees)
P5 = spec.Params(5, 36, F(10.0), F(25.0), F(0.0), F(2.5), F(0.1), 4, 0)
# 8 rings of 1 degree from -4.5: adjacent rings are close enough for a step of a few degrees between them
P8 = spec.Params(8, 64, F(1.0), F(4.5), F(0.0), F(2.5), F(0.1), 7, 0)
# 6 rings of 5 degrees centred on -25 ... 0: three on the ground, three on a wall
PW = spec.Params(6, 36, F(5.0), F(27.5), F(0.0), F(2.5), F(0.1), 5, 0)
P2 = spec.Params(2, 4, F(30.0), F(30.0), F(0.0), F(10.0), F(0.1), 1, 1)
GRIDS = {"2x4": P2, "5x36": P5, "8x64": P8, "64x4500": spec.DEFAULT}


def _pts(rows):
    xyz = np.asarray(rows, F).reshape(-1, 3)
    return np.ascontiguousarray(np.concatenate([xyz, np.full((len(xyz), 1), 0.5, F)], axis=1))


def polar(elev_deg, az_deg, rng=5.0):
    """(x, y, z) at an elevation, an azimuth atan2(y, x) and a range, computed in double."""
    e, a = np.deg2rad(elev_deg), np.deg2rad(az_deg)
    return (rng * np.cos(e) * np.cos(a), rng * np.cos(e) * np.sin(a), rng * np.sin(e))


@functools.lru_cache(maxsize=None)
def tables(p):
    return spec.tables(p)


def _case(name, points, p):
    points = np.ascontiguousarray(points, dtype=F).reshape(-1, 4)
    tab = tables(p)
    return {"name": name, "points": points, "params": p, "tab": tab, "want": spec.mark(points, p, tab)}


# ---- cell geometry --------------------------------------------------------------------------------------------------
def _geometry_cases():
    out = []
    tab = tables(P5)
    T, Cc, S = tab["T"], tab["C"], tab["S"]
    # z == T[r] * h exactly (h = 2: the product only shifts the exponent) lands in ring r, one ulp below in r - 1; at the top
    # border, T[n_rings], the point is out
    rows = []
    for r in range(P5.n_rings + 1):
        z = F(T[r] * F(2))
        rows += [(2.0, 0.0, z), (2.0, 0.0, down(z))]
    c = _case("ring_borders_exact", _pts(rows), P5)
    ring, why = c["want"]["cells"]["ring"], c["want"]["cells"]["why"]
    for r in range(P5.n_rings + 1):
        assert F(np.sqrt(F(F(2) * F(2)))) == F(2)
        assert (ring[2 * r], why[2 * r]) == ((r, 0) if r < P5.n_rings else (-1, 5)), (r, ring[2 * r], why[2 * r])
        assert (ring[2 * r + 1], why[2 * r + 1]) == ((r - 1, 0) if r > 0 else (-1, 4)), (r, ring[2 * r + 1])
    out.append(c)
    # a point ON a column border, (2 C[c], 2 S[c]): both products are equal, the border belongs to the cell it opens; turned back
    # by 1e-4 rad it is in the cell before (one ulp of a coordinate need not move a rounded product)
    rows, cols = [], []
    for col in (19, 22, 27, 31, 35, 0, 4, 9, 13, 18):                           # some in every quadrant, the first and the last
        x, y = F(F(2) * Cc[col]), F(F(2) * S[col])
        assert F(Cc[col] * y) == F(S[col] * x)
        rows += [(x, y, 0.0), (float(x) * np.cos(1e-4) + float(y) * np.sin(1e-4), float(y) * np.cos(1e-4) - float(x) * np.sin(1e-4), 0.0)]
        cols.append(col)
    c = _case("column_borders_exact", _pts(rows), P5)
    got = c["want"]["cells"]["col"]
    for i, col in enumerate(cols):
        assert got[2 * i] == col and got[2 * i + 1] == (col - 1) % P5.n_columns, (col, got[2 * i], got[2 * i + 1])
    assert set(spec.quadrant(c["points"][::2, 0], c["points"][::2, 1])) == {0, 1, 2, 3}
    out.append(c)
    # one point per quadrant and on each half axis, in the middle of their cells: the columns of the reference's formula
    az = [30.0, 120.0, 210.0, 300.0, 0.0, 90.0, 180.0, 270.0]
    c = _case("quadrants_and_axes", _pts([polar(0.0, a) for a in az[:4]] + [(3, 0, 0), (0, 3, 0), (-3, 0, 0), (0, -3, 0)]), P5)
    cl = c["want"]["cells"]
    assert list(spec.quadrant(c["points"][:, 0], c["points"][:, 1])) == [0, 1, 2, 3, 0, 1, 2, 3]
    assert list(cl["col"]) == [21, 30, 3, 12, 18, 27, 0, 9]          # round(azimuth / 10) + 18, wrapped
    assert np.all(cl["why"] == 0) and np.all(cl["ring"] == 2)
    out.append(c)
    # the cell that straddles a quadrant's edge: a point just inside the new quadrant counts no border of its run, k = 0, and
    # lands in the cell that began in the quadrant before
    c = _case("straddling_cells_k0", _pts([polar(0.0, 1.0), polar(0.0, 91.0), polar(0.0, 181.0), polar(0.0, 271.0)]), P5)
    cl = c["want"]["cells"]
    assert list(cl["k"]) == [0, 0, 0, 0] and list(cl["col"]) == [18, 27, 0, 9]
    assert [int(tab["first"][q]) for q in range(4)] == [19, 28, 1, 10]
    out.append(c)
    # the wrap: cell n_columns - 1 ends and cell 0 begins at 175 degrees; quadrant 1's run of borders wraps from 35 to 0
    c = _case("wrap_cells", _pts([polar(0.0, 170.0), polar(0.0, 174.9), polar(0.0, 175.1), polar(0.0, 178.0), (-3, 0, 0),
                                  polar(0.0, -178.0), polar(0.0, -174.9)]), P5)
    cl = c["want"]["cells"]
    assert list(cl["col"]) == [35, 35, 0, 0, 0, 0, 1]
    assert int(tab["first"][1]) + int(tab["len"][1]) - 1 == 36                     # the run's last border is column 0
    out.append(c)
    return out


# ---- points with no cell ----------------------------------------------------------------------------------------------
def _no_cell_case():
    mr = F(P5.min_range)
    rows = [(0.0, 0.0, 1.0), (0.0, -0.0, -1.0), (1e-30, 1e-30, 0.0),                  # h == 0 (the last: x x underflows)
            (np.nan, 1, 0), (1, np.nan, 0), (1, 1, np.nan), (np.inf, 1, 0), (1, -np.inf, 0), (1, 1, np.inf), (np.inf, 1, np.inf),
            (down(mr), 0.0, 0.0), (mr, 0.0, 0.0),                                      # range just below and at min_range
            polar(-30.0, 40.0), polar(26.0, 40.0), polar(-24.0, 40.0), polar(24.0, 40.0),   # ring -1, ring n_rings, rings 0 and 4
            (1e30, 1.0, 0.0)]                                                        # finite, h overflows to inf: still a cell
    c = _case("no_cell", _pts(rows), P5)
    why, ring = c["want"]["cells"]["why"], c["want"]["cells"]["ring"]
    assert list(why) == [2, 2, 2, 1, 1, 1, 1, 1, 1, 1, 3, 0, 4, 5, 0, 0, 0], list(why)
    assert list(ring[-5:-1]) == [-1, -1, 0, 4] and ring[-1] == 2
    assert list(c["want"]["flags"]) == [2] * 11 + [0, 2, 2, 0, 0, 0]
    assert c["want"]["counts"][0] == 4
    return c


# ---- later point wins -------------------------------------------------------------------------------------------------
def _later_wins_cases():
    """Ground at z = -1 seen in rings 0 and 1 (elevations -20 and -10 degrees) of column 18; a second point on ring 0's ray at half
    the range, z = -0.5, makes the step to ring 1 too steep.  Whichever of the two comes LAST decides for every point of the cell."""
    g0, g1 = (1.0 / np.tan(np.deg2rad(20.0)), 0.0, -1.0), (1.0 / np.tan(np.deg2rad(10.0)), 0.0, -1.0)
    near = (0.5 * g0[0], 0.0, -0.5)
    out = []
    for name, rows, winner, flag in (("later_wins_two_level", [near, g1, g0], 2, 1), ("later_wins_two_steep", [g0, g1, near], 2, 0),
                                     ("later_wins_three", [near, g0, g1, (g0[0], 0.01, -1.0), near, (g0[0], -0.01, -1.0)], 5, 1)):
        c = _case(name, _pts(rows), P5)
        w = c["want"]
        ring0 = [i for i in range(len(rows)) if w["cells"]["ring"][i] == 0]
        assert len(ring0) == len(rows) - 1 and len(set(w["cells"]["cell"][ring0])) == 1
        assert w["winner"][0, 18] == winner and w["state"][0, 18] == flag
        assert all(w["flags"][i] == flag for i in ring0)                    # every point of the cell, not only the winner
        assert w["counts"][0] == len(rows) and w["counts"][1] == 2 and w["counts"][3] == flag * len(ring0)
        out.append(c)
    return out


# ---- cell states ------------------------------------------------------------------------------------------------------
def _slope_pair(p, slope, toward):
    """A lower point (x, 0, zl) and an upper one (x + hd, 0, zu) in rings r and r + 1 of one column, hd a power of two, with
    zu - zl == slope * hd EXACTLY in float32, and the same pair with zu - zl one ulp further `toward`.  Found by trying: the sum
    zl + dz has to be exact for both, and the two elevations one ring apart."""
    tab = tables(p)
    zl = np.linspace(-0.6, 0.3, 9001).astype(F)
    col = lambda x, z: _pts(np.stack([np.full_like(z, x), np.zeros_like(z), z], 1))      # noqa: E731
    for hd in (1.0, 2.0, 4.0, 0.5, 0.25):
        for x in (2.0, 1.0, 3.0, 4.0, 6.0):
            dz = F(F(slope) * F(hd))
            dz2 = np.nextafter(dz, F(toward))
            zu, zu2 = (zl + dz).astype(F), (zl + dz2).astype(F)
            exact = ((zu - zl).astype(F) == dz) & ((zu2 - zl).astype(F) == dz2)
            lo, hi, hi2 = spec.cells(col(x, zl), p, tab), spec.cells(col(x + hd, zu), p, tab), spec.cells(col(x + hd, zu2), p, tab)
            good = exact & (lo["why"] == 0) & (hi["why"] == 0) & (hi2["why"] == 0) & (hi["ring"] == lo["ring"] + 1) & \
                (hi2["ring"] == hi["ring"]) & (lo["ring"] < p.ground_rings) & (lo["col"] == hi["col"])
            if good.any():
                i = np.flatnonzero(good)[0]
                assert F(np.sqrt(F(F(hd) * F(hd)))) == F(hd)
                return int(lo["ring"][i]), int(lo["col"][i]), (x, 0.0, zl[i]), (x + hd, 0.0, zu[i]), (x + hd, 0.0, zu2[i])
    raise AssertionError("no exact pair")


def _state_cases():
    out = []
    tab = tables(P8)
    for name, slope, toward, inside in (("slope_at_thi", tab["thi"], np.inf, 1), ("slope_at_tlo", tab["tlo"], -np.inf, 1)):
        r, col, low, at, over = _slope_pair(P8, slope, toward)
        c = _case(name + "_exactly", _pts([low, at]), P8)
        assert c["want"]["state"][r, col] == 1 and list(c["want"]["flags"]) == [1, 0]
        out.append(c)
        c = _case(name + "_one_ulp_over", _pts([low, over]), P8)
        assert c["want"]["state"][r, col] == 0 and list(c["want"]["flags"]) == [0, 0]
        out.append(c)
    # the cell above empty: -1, and the point is not ground; so is every empty cell below ground_rings, and 0 at and above it
    c = _case("upper_cell_empty", _pts([polar(-20.0, 0.0)]), P5)
    w = c["want"]
    assert w["state"][0, 18] == -1 and list(w["flags"]) == [0]
    assert np.all(w["state"][:4] == -1) and np.all(w["state"][4] == 0)
    out.append(c)
    # two points one above the other: hd == 0 and dz > 0, not level whatever the tolerance
    c = _case("stacked_points_hd_zero", _pts([(3.0, 0.0, 3.0 * np.tan(np.deg2rad(-20.0))), (3.0, 0.0, 3.0 * np.tan(np.deg2rad(-10.0)))]), P5)
    assert c["want"]["state"][0, 18] == 0 and c["want"]["cells"]["ring"].tolist() == [0, 1]
    out.append(c)
    # ground, then a wall, in one column (PW): rings 0 ... 2 on z = -1, rings 3 ... 5 on x = 4.  Without mark_upper the last ground
    # cell stays unmarked (its step goes up the wall); with it the step below marks it.  ground_rings 0 marks nothing and calls
    # nothing empty; ground_rings n_rings - 1 is the most
    ground = [(1.0 / np.tan(np.deg2rad(e)), 0.0, -1.0) for e in (25.0, 20.0, 15.0)]
    wall = [(4.0, 0.0, 4.0 * np.tan(np.deg2rad(e))) for e in (-10.0, -5.0, 0.0)]
    for name, p, want in (("ground_then_wall", PW, [1, 1, 0, 0, 0, 0]), ("ground_then_wall_mark_upper", PW._replace(mark_upper=1), [1, 1, 1, 0, 0, 0]),
                          ("ground_rings_0", PW._replace(ground_rings=0, mark_upper=1), [0] * 6),
                          ("ground_rings_1_mark_upper", PW._replace(ground_rings=1, mark_upper=1), [1, 1, 0, 0, 0, 0]),
                          ("ground_rings_2", PW._replace(ground_rings=2), [1, 1, 0, 0, 0, 0])):
        c = _case(name, _pts(ground + wall), p)
        w = c["want"]
        assert list(w["cells"]["ring"]) == [0, 1, 2, 3, 4, 5] and set(w["cells"]["col"]) == {18}
        assert list(w["state"][:, 18]) == want and list(w["flags"]) == want, (name, list(w["state"][:, 18]))
        assert np.all(w["state"][:p.ground_rings, 17] == -1) and np.all(w["state"][p.ground_rings:, 17] == 0)
        out.append(c)
    assert PW.ground_rings == PW.n_rings - 1
    return out


def identical_points_pair():
    """hd == dz == 0: the pair test itself says level (0 >= tlo * 0 and 0 <= thi * 0).  No two cells share a point, so no scan
    reaches it; it is asserted on the restatement's pair function with a hand-made winner image."""
    pts = _pts([(3.0, 1.0, -1.0)])
    winner = np.zeros((P5.n_rings, P5.n_columns), np.int64)
    return spec.pair_states(pts, winner, P5, tables(P5))


# ---- sizes ------------------------------------------------------------------------------------------------------------
def random_points(rng, n, bad=True):
    pts = np.zeros((n, 4), F)
    pts[:, :2] = rng.normal(0.0, 10.0, (n, 2))
    pts[:, 2] = rng.normal(-0.5, 1.5, n)
    pts[:, 3] = rng.uniform(0, 1, n)
    if bad and n >= 16:                       # a few of every kind without a cell
        i = rng.choice(n, 6, replace=False)
        pts[i[0], 0] = np.nan
        pts[i[1], 2] = np.inf
        pts[i[2], :2] = 0.0
        pts[i[3], :3] = 0.01
        pts[i[4], 2] = 200.0
        pts[i[5], 2] = -200.0
    return pts


def _size_cases():
    out = []
    for grid, p in GRIDS.items():
        for n in (0, 1, 255, 256, 257, 4097):
            rng = np.random.default_rng(1000 + n + p.n_columns)
            c = _case(f"count_{n}_{grid}", random_points(rng, n), p)
            w = c["want"]
            assert len(w["flags"]) == n and w["counts"][0] <= n and w["counts"][1] <= w["counts"][0]
            if n >= 255:
                assert w["counts"][0] > n // 3 and np.count_nonzero(w["flags"] == 2) >= 6
                if grid != "64x4500":
                    assert w["counts"][0] > w["counts"][1]                     # cells shared: later wins decides something
            if n >= 255 and grid == "5x36":
                shared = w["counts"][0] - w["counts"][1]
                assert 0.25 * w["counts"][0] < shared, (shared, w["counts"])
            out.append(c)
    return out


@functools.lru_cache(maxsize=None)
def small_cases():
    """Every named case, in a fixed order."""
    return tuple(_geometry_cases() + [_no_cell_case()] + _later_wins_cases() + _state_cases() + _size_cases())


@functools.lru_cache(maxsize=None)
def random_case(seed):
    """A random scan under random valid parameters."""
    rng = np.random.default_rng(4200 + seed)
    nr, nc = int(rng.integers(2, 40)), int(rng.integers(4, 700))
    res = F(rng.uniform(0.3, min(3.0, 80.0 / nr)))
    bottom = F(rng.uniform(0.2, 0.9) * nr * float(res))
    p = spec.Params(nr, nc, res, bottom, F(rng.uniform(-5, 5)), F(rng.uniform(0.0, 12.0)), F(rng.uniform(0.0, 2.0)),
                    int(rng.integers(0, nr)), int(rng.integers(0, 2)))
    n = int(rng.integers(1, 5000))
    pts = random_points(rng, n)
    pts[:, 2] = (np.hypot(pts[:, 0], pts[:, 1]) * np.tan(np.deg2rad(rng.uniform(-float(bottom) - 2, nr * float(res) - float(bottom) + 2, n)))).astype(F)
    flat = rng.uniform(size=n) < 0.5                     # half of them on a plane: level steps exist
    pts[flat, 2] = F(-1.2)
    c = _case(f"random_{seed}", pts, p)
    return c


INVALID = [dict(n_rings=1), dict(n_rings=129), dict(n_columns=3), dict(n_columns=16385), dict(ang_res_y=float("nan")),
           dict(ang_bottom=float("inf")), dict(mount_deg=float("nan")), dict(tol_deg=float("inf")), dict(min_range=float("nan")),
           dict(ang_res_y=0.0), dict(ang_res_y=-1.0), dict(ang_bottom=90.0), dict(ang_bottom=-64.0), dict(ang_res_y=1.7),
           dict(mount_deg=88.0), dict(mount_deg=-88.0, tol_deg=2.0), dict(tol_deg=-0.1), dict(tol_deg=90.0), dict(min_range=-0.1),
           dict(ground_rings=-1), dict(ground_rings=64), dict(mark_upper=2), dict(mark_upper=-1)]


# ---- the street scan ----------------------------------------------------------------------------------------------------
def is_ground_truth(points):
    """kitti_scan's ground plane lies 1.73 m under the sensor."""
    return np.abs(np.asarray(points, np.float64)[:, 2] + 1.73) < 1e-3


@functools.lru_cache(maxsize=None)
def kitti_marks(which):
    """The restatement on scan_cases.kitti_scan(): which = "default", "hdl64e" or "hdl64e_upper"."""
    p = {"default": spec.DEFAULT, "hdl64e": spec.HDL64E, "hdl64e_upper": spec.HDL64E._replace(mark_upper=1)}[which]
    return _case("kitti_" + which, scan_cases.calibration_case()["points"], p)


# ---- fusing -------------------------------------------------------------------------------------------------------------
# 64 beams from +24 to -24 degrees, 720 firings: each beam at its ring's centre, each firing in a column of its own
_FUSE_RES = F(48.0) / F(63.0)
FUSE_GROUND = spec.Params(64, 720, _FUSE_RES, F(24.0) + _FUSE_RES / F(2.0), F(0.0), F(2.5), F(0.1), 63, 1)


@functools.lru_cache(maxsize=None)
def fuse_frames():
    """scan_cases.fuse_frames()' scene, poses and 48 x 40 x 36 grid with a room around the sensor, its floor 0.3 m below it: the
    floor passes through the grid under the sphere, and every ray returns.  ([(cam2world, points, flags under FUSE_GROUND)],
    velo2img)."""
    scene = synth.SurfScene(scan_cases.FUSE_DIMS, scan_cases.FUSE_VS, scan_cases.FUSE_ORIGIN, K=scan_cases.FUSE_K, h=scan_cases.FUSE_H,
                            w=scan_cases.FUSE_W)
    _, velo2img = scan_cases.fuse_frames()
    frames = []
    for k in (0, 2, 5):
        c2w = scene.pose(k, n=8)
        pts = synth.lidar_scan(scene, c2w, n_azimuth=720, elev_deg=(24.0, -24.0), room=(3.0, 3.0, 2.0, 0.3))
        assert len(pts) == 64 * 720
        w = spec.mark(pts, FUSE_GROUND, tables(FUSE_GROUND))
        floor = np.abs(pts[:, 2].astype(np.float64) + 0.3) < 1e-4
        assert np.count_nonzero(floor) > 5000 and np.all(w["flags"][floor] == 1)      # the floor is found, all of it
        assert 0.2 < np.mean(w["flags"] == 1) < 0.8 and not np.any(w["flags"] == 2)
        frames.append((c2w, pts, w["flags"]))
    return tuple(frames), velo2img


def restated_depth(points, flags, which, velo2img, fill=None):
    """The z-depth image of the fuse frames' size that the selecting calls make: the kept points projected, then filled or not."""
    kept = spec.select(points, flags, which)
    depth = scan_spec.scan_depth(kept, velo2img, scan_cases.FUSE_K, scan_cases.FUSE_H, scan_cases.FUSE_W)
    return depth if fill is None else scan_fill_spec.fill(depth, *fill)[0]
