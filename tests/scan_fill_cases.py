"""The named cases of the lidar gap fill (test infrastructure, no GPU): the smallest images at which the kernel of
csrc/tsdf_scan_fill.hip.h can go wrong.  Each case is built once, asserts here, on the CPU, that the restatement
(tests/scan_fill_spec.py) reaches the branch it is named for, and carries the restatement's images;
tests/test_scan_fill_spec.py runs the assertions, tests/test_gpu_scan_fill.py holds the device to the images bit for bit.

The kernel's tile is TILE_W x TILE_H = 64 x 8 pixels (kFillTileW, kFillTileH of the header), its halo at most 15: the shapes
below are one tile exactly (8 x 64), a few tiles and a bit in both directions (37 x 70), a single row and a single column
(1 x 300, 300 x 1) and sixteen tiles and a bit down by two tiles and a bit across (130 x 131)."""
import functools

import numpy as np

import scan_cases
import scan_fill_spec as spec

F = np.float32
TILE_W, TILE_H = 64, 8
SHAPES = ((37, 70), (1, 300), (300, 1), (130, 131), (TILE_H, TILE_W))
H, W = 37, 70

up = lambda a: np.nextafter(F(a), F(np.inf))          # noqa: E731


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def _case(name, depth, su=5, sv=8, jump=F(0.05)):
    depth = np.ascontiguousarray(depth, F)
    filled, kind, n = spec.fill(depth, su, sv, jump)
    return {"name": name, "depth": depth, "params": (int(su), int(sv), float(F(jump))), "filled": filled, "kind": kind,
            "n_filled": n, "H": depth.shape[0], "W": depth.shape[1]}


def sparse_image(h, w, seed, density=0.15, specials=True):
    """A smooth surface with a step in it, kept at `density` of the pixels, with a few values that are no sources."""
    rng = np.random.default_rng(seed)
    v, u = np.mgrid[0:h, 0:w]
    d = (2.0 + 0.004 * u + 0.007 * v + np.where(u + 2 * v > (w + 2 * h) * 0.6, 0.5, 0.0)).astype(F)
    d = np.where(rng.random((h, w)) < density, d, F(0)).astype(F)
    if specials and h * w >= 64:
        flat = d.reshape(-1)
        at = rng.choice(h * w, 6, replace=False)
        flat[at] = np.array([np.nan, -1.0, np.inf, -np.inf, 1e-40, -0.0], F)
    return d


def empty(h=H, w=W):
    return np.zeros((h, w), F)


# ---- the passes switched off ----------------------------------------------------------------------------------------
def _identity_cases():
    out = []
    d = sparse_image(H, W, 1, 0.4)
    for su, sv in ((0, 0), (1, 1), (0, 1), (1, 0)):
        c = _case(f"spans_{su}_{sv}_identity", d, su, sv)
        assert c["n_filled"] == 0 and np.array_equal(bits(c["filled"]), bits(d))
        assert np.array_equal(c["kind"] == spec.MEASURED, spec.is_source(d)) and not np.any(c["kind"] >= 2)
        out.append(c)
    assert _case("_", d, 5, 8)["n_filled"] > 100             # the same image with the passes on is not the identity
    # one pass on, the other off
    cu, cv = _case("u_pass_alone", d, 5, 0), _case("v_pass_alone", d, 0, 8)
    assert np.any(cu["kind"] == 2) and not np.any(cu["kind"] == 3) and np.any(cv["kind"] == 3) and not np.any(cv["kind"] == 2)
    return out + [cu, cv]


# ---- distances ------------------------------------------------------------------------------------------------------
def _distance_cases():
    out = []
    for span in (2, 5, 16):
        d = empty()
        d[3, 10] = d[3, 10 + span] = F(2)                       # exactly max_span apart: bridged
        d[7, 40] = d[7, 40 + span + 1] = F(2)                   # one more: not
        c = _case(f"distance_u_span_{span}", d, span, 0)
        assert np.all(c["kind"][3, 11:10 + span] == 2) and np.all(bits(c["filled"][3, 11:10 + span]) == bits(F(2)))
        assert c["n_filled"] == span - 1
        out.append(c)
        dv = empty()
        dv[3, 10] = dv[3 + span, 10] = F(3)
        dv[7, 40] = dv[7 + span + 1, 40] = F(3)
        c = _case(f"distance_v_span_{span}", dv, 0, span)
        assert np.all(c["kind"][4:3 + span, 10] == 3) and np.all(bits(c["filled"][4:3 + span, 10]) == bits(F(3)))
        assert c["n_filled"] == span - 1
        out.append(c)
    # the nearer source wins over a farther one, on both sides
    d = empty()
    d[5, 5], d[5, 7], d[5, 10], d[5, 12] = F(2.0), F(2.02), F(2.04), F(2.06)
    c = _case("nearer_source_wins", d, 8, 0)
    want, _ = spec.fill_line_pass(np.array([[2.02, 0, 0, 2.04]], F), 8, F(0.05))
    far, _ = spec.fill_line_pass(np.array([[2.0, 0, 0, 0, 0, 2.04]], F), 8, F(0.05))
    assert np.array_equal(bits(c["filled"][5, 8:10]), bits(want[0, 1:3])) and bits(far[0, 3]) != bits(want[0, 1])
    assert c["kind"][5, 6] == 2 and c["kind"][5, 11] == 2 and c["n_filled"] == 4
    out.append(c)
    # a source on one side only: nothing is extrapolated
    d = empty()
    d[5, 20] = d[20, 5] = F(2)
    c = _case("one_side_only", d, 16, 16)
    assert c["n_filled"] == 0 and np.array_equal(bits(c["filled"]), bits(d))
    out.append(c)
    return out


# ---- the image's and the lines' ends ----------------------------------------------------------------------------------
def _border_cases():
    out = []
    # the last pixels of a row and a source at the start of the next: two pixels apart in memory, no pair
    d = empty()
    d[4, W - 3] = d[5, 0] = d[5, 1] = F(2)
    d[9, W - 1] = d[10, 0] = F(2)
    c = _case("row_does_not_wrap", d, 8, 0)
    assert c["n_filled"] == 0 and np.array_equal(bits(c["filled"]), bits(d))
    assert spec.fill_line_pass(d.reshape(1, -1), 8, F(0.05))[1].sum() == 2       # read as ONE line the gap would close
    out.append(c)
    # sources two pixels inside each border: the pixels between them and the border stay empty;
    # sources ON the border pixels are sources like any other
    d = empty()
    d[10, 2] = d[10, W - 3] = d[2, 30] = d[H - 3, 30] = F(2)
    d[20, 0] = d[20, 3] = d[22, W - 4] = d[22, W - 1] = F(2)
    d[0, 50] = d[3, 50] = d[H - 4, 52] = d[H - 1, 52] = F(2)
    c = _case("image_borders", d, 5, 5)
    k = c["kind"]
    assert not np.any(k[10] >= 2) and not np.any(k[:, 30] >= 2)
    assert np.all(k[20, 1:3] == 2) and np.all(k[22, W - 3:W - 1] == 2) and np.all(k[1:3, 50] == 3) and np.all(k[H - 3:H - 1, 52] == 3)
    assert c["n_filled"] == 8
    out.append(c)
    return out


# ---- the depth jump ---------------------------------------------------------------------------------------------------
def _jump_cases():
    out = []
    half = F(0.5)
    d = empty()
    d[3, 10], d[3, 12] = F(2), F(3)                 # |a - b| = 1 = 0.5 * 2 exactly: bridged
    d[8, 10], d[8, 12] = F(2), up(3)                # one ulp above: not
    d[13, 10], d[13, 12] = F(3), F(2)               # the same from the other side
    d[18, 10], d[18, 12] = up(3), F(2)
    d[25, 30], d[27, 30] = F(2), F(3)               # ... and along a column
    d[25, 40], d[27, 40] = F(2), up(3)
    with np.errstate(all="ignore"):
        assert F(3) - F(2) == half * F(2) and np.abs(F(2) - up(3)) > half * F(2)
    c = _case("jump_exact_and_one_ulp_above", d, 4, 4, half)
    k = c["kind"]
    assert k[3, 11] == 2 and k[13, 11] == 2 and k[26, 30] == 3 and k[8, 11] == 0 and k[18, 11] == 0 and k[26, 40] == 0
    assert c["n_filled"] == 3 and abs(float(c["filled"][3, 11]) - 2.4) < 1e-6
    out.append(c)
    d = empty()
    d[3, 10], d[3, 12], d[10, 20], d[12, 20] = F(2), F(3), F(3), F(2)
    d[20, 10], d[20, 12] = F(2), F(2.1)             # exactly at 5 % in exact arithmetic, decided by the float32 operations
    c = _case("two_against_three_at_default_jump", d, 5, 8)
    assert c["kind"][3, 11] == 0 and c["kind"][11, 20] == 0
    out.append(c)
    c = _case("jump_rel_zero", np.where(sparse_image(H, W, 3, 0.3, False) > 0, F(2.5), F(0)), 5, 8, F(0))
    assert c["n_filled"] > 100                       # equal values pass |a - b| <= 0
    out.append(c)
    return out


# ---- what the v pass reads --------------------------------------------------------------------------------------------
def _pass_order_cases():
    out = []
    d = empty()
    d[5, 10] = d[5, 13] = d[9, 10] = d[9, 13] = F(2)
    c = _case("v_pass_fed_by_u_filled", d, 5, 8)
    k = c["kind"]
    assert np.all(k[5, 11:13] == 2) and np.all(k[9, 11:13] == 2) and np.all(k[6:9, 11:13] == 3) and np.all(k[6:9, 10] == 3)
    assert c["n_filled"] == 4 + 12
    out.append(c)
    # (4, 11) lies between two v-filled pixels of its row that agree, and has no source above it in its column: it stays
    # empty, where a u pass run again over the output would fill it
    d = empty()
    d[2, 10], d[5, 10], d[8, 10] = F(2.0), F(2.075), F(2.15)
    d[2, 12], d[5, 12], d[8, 12] = F(2.15), F(2.075), F(2.0)
    c = _case("v_pass_not_fed_by_v_filled", d, 4, 4)
    k = c["kind"]
    assert k[4, 10] == 3 and k[4, 12] == 3 and k[5, 11] == 2 and k[2, 11] == 0 and k[8, 11] == 0
    assert k[4, 11] == 0 and k[3, 11] == 0 and k[6, 11] == 0
    assert spec.fill_line_pass(c["filled"], 4, F(0.05))[1][4, 11]
    out.append(c)
    return out


# ---- values that are no sources -------------------------------------------------------------------------------------
def _value_cases():
    out = []
    odd = np.array([0x7FC01234, 0xFFC00001, 0x7F800001, 0xBF800000, 0x7F800000, 0xFF800000, 0x00000000, 0x80000000], np.uint32).view(F)
    d = empty()
    for i, val in enumerate(odd):                # each beside a source; the sources differ by 20 % and more, so none pairs up
        d[4 * i + 2, 10], d[4 * i + 2, 11] = F(2 * 1.2 ** i), val
        d[2, 30 + 4 * i], d[3, 30 + 4 * i] = F(2 * 1.2 ** (8 + i)), val
    c = _case("non_sources_keep_their_bits", d, 16, 16)
    assert c["n_filled"] == 0 and np.array_equal(bits(c["filled"]), bits(d))
    assert not np.any(spec.is_source(odd)) and np.count_nonzero(c["kind"] == 1) == 16
    out.append(c)
    # an empty pixel of any bits between two sources is filled like a zero
    d = empty()
    for i, val in enumerate(odd):
        d[4 * i + 2, 10], d[4 * i + 2, 11], d[4 * i + 2, 12] = F(2), val, F(2)
    c = _case("non_sources_between_sources", d, 2, 0)
    assert c["n_filled"] == 8 and np.all(bits(c["filled"][2::4, 11][:8]) == bits(F(2)))
    out.append(c)
    # FLT_MAX on both sides: denormal reciprocals; denormal sources
    d = empty()
    d[3, 10] = d[3, 12] = spec.FLT_MAX
    d[6, 10] = d[6, 13] = F(1e-38)
    d[9, 10] = d[9, 12] = F(1e-40)
    with np.errstate(all="ignore"):
        r = F(1) / spec.FLT_MAX
        assert 0 < r < np.finfo(F).tiny and F(1e-38) < np.finfo(F).tiny and F(1) / F(1e-40) == F(np.inf)
    c = _case("flt_max_and_denormal_sources", d, 4, 0)
    assert c["kind"][3, 11] in (0, 2) and c["kind"][9, 11] == 0       # 1 / 1e-40 = inf: inv = inf, d = 0 is refused
    assert np.all(c["kind"][6, 11:13] == 2) and np.all(c["filled"][6, 11:13] < np.finfo(F).tiny)
    out.append(c)
    return out


# ---- pairs across the tile's borders --------------------------------------------------------------------------------
def _tile_cases():
    h, w = 130, 131
    d = empty(h, w)
    # u pass, a source on each side of the column border 63 | 64 (and 127 | 128), in the first and in a later tile row
    for v in (3, 45, 77, 120):
        d[v, TILE_W - 2], d[v, TILE_W + 1] = F(2), F(2.02)
        d[v, 2 * TILE_W - 1], d[v, 2 * TILE_W + 2] = F(3), F(3.03)
    # v pass, a source on each side of the row border 7 | 8 (and 63 | 64), in columns on either side of a column border
    for u in (5, TILE_W - 1, TILE_W, 130):
        d[TILE_H - 2, u], d[TILE_H + 2, u] = F(4), F(4.04)
        d[8 * TILE_H - 1, u], d[8 * TILE_H + 1, u] = F(5), F(5.05)
    # v pass across a row border, fed by u-filled pixels of the other tile's rows
    d[2 * TILE_H - 3, 30] = d[2 * TILE_H - 3, 33] = d[2 * TILE_H + 2, 30] = d[2 * TILE_H + 2, 33] = F(6)
    # the longest reach: 15 pixels into the neighbour tile, both passes
    d[50, TILE_W - 1], d[50, TILE_W + 15] = F(7), F(7.07)
    d[3 * TILE_H + 15, 100], d[3 * TILE_H - 1, 100] = F(8), F(8.08)
    c = _case("pairs_across_tile_borders", d, 16, 16)
    k = c["kind"]
    for v in (3, 45, 77, 120):
        assert np.all(k[v, TILE_W - 1:TILE_W + 1] == 2) and np.all(k[v, 2 * TILE_W:2 * TILE_W + 2] == 2)
    for u in (5, TILE_W - 1, TILE_W, 130):
        assert np.all(k[TILE_H - 1:TILE_H + 2, u] == 3) and k[8 * TILE_H, u] == 3
    assert np.all(k[2 * TILE_H - 2:2 * TILE_H + 2, 31:33] == 3) and np.all(k[2 * TILE_H - 3, 31:33] == 2)
    assert np.all(k[50, TILE_W:TILE_W + 15] == 2) and np.all(k[3 * TILE_H:3 * TILE_H + 15, 100] == 3)
    return [c]


# ---- whole images ---------------------------------------------------------------------------------------------------
def _whole_image_cases():
    out = []
    c = _case("all_empty", empty(), 16, 16)
    assert c["n_filled"] == 0 and not c["kind"].any() and not bits(c["filled"]).any()
    out.append(c)
    full = (2.0 + 0.01 * np.arange(H * W).reshape(H, W)).astype(F)
    c = _case("all_measured", full, 16, 16)
    assert c["n_filled"] == 0 and np.all(c["kind"] == 1) and np.array_equal(bits(c["filled"]), bits(full))
    out.append(c)
    for i, (h, w) in enumerate(SHAPES):
        for su, sv, dens in ((16, 16, 0.02), (5, 8, 0.15)):
            c = _case(f"sparse_{h}x{w}_spans_{su}_{sv}", sparse_image(h, w, 10 + i, dens if h * w > 400 else 0.2), su, sv)
            k = c["kind"]
            if w > 1:
                assert np.any(k == 2), c["name"]
            if h > 1:
                assert np.any(k == 3), c["name"]
            if h == 1:
                assert not np.any(k == 3)
            if w == 1:
                assert not np.any(k == 2)
            assert np.any(k == 0) and np.array_equal(k == 1, spec.is_source(c["depth"]))
            out.append(c)
    return out


@functools.lru_cache(maxsize=None)
def small_cases():
    """Every small case, in a fixed order."""
    out = (_identity_cases() + _distance_cases() + _border_cases() + _jump_cases() + _pass_order_cases() + _value_cases() +
           _tile_cases() + _whole_image_cases())
    assert len({c["name"] for c in out}) == len(out)
    return tuple(out)


@functools.lru_cache(maxsize=None)
def kitti_case():
    """The 375 x 1242 depth image of the calibration scan (scan_cases.calibration_case), default parameters."""
    c = scan_cases.calibration_case()
    k = _case("kitti_calibration_filled", c["depth"], *spec.DEFAULT)
    assert k["H"] == scan_cases.KITTI_H and k["W"] == scan_cases.KITTI_W
    return k


def random_case(seed):
    """One of the random sweep: a shape of SHAPES, random parameters, a random sparse image."""
    rng = np.random.default_rng(1000 + seed)
    h, w = SHAPES[seed % len(SHAPES)]
    su, sv = int(rng.integers(0, 17)), int(rng.integers(0, 17))
    jump = F(rng.choice([0.0, 0.01, 0.05, 0.3, 1e30]))
    return _case(f"random_{seed}", sparse_image(h, w, 2000 + seed, float(rng.uniform(0.03, 0.5))), su, sv, jump)
