"""The ground rule's restatement (tests/scan_ground_spec.py) on the CPU: its cells are the reference's formula's wherever float32
cannot tell (and, as it happens, everywhere), its level test is the reference's angle test, every named case of
tests/scan_ground_cases.py reaches the branch it is named for (the cases assert that as they are built), a second, scalar
statement of the rule gives the same results, the street scan's ground is found, and a fused object volume loses the road under
it.  The library's host-only table builder is swept by a stand-alone sanitized program.  tests/test_gpu_scan_ground.py holds the
device to the same results."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import scan_cases
import scan_fill_cases
import scan_fill_spec
import scan_ground_cases as cases
import scan_ground_spec as spec
import scan_spec
from semantic_slam_amd import capi, synth

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- parameters and tables ------------------------------------------------------------------------------------------------
def test_default_parameters_are_the_reference_literals():
    p = capi.scan_ground_params_default()
    assert spec.params(p) == spec.DEFAULT
    assert (p.n_rings, p.n_columns, p.ground_rings, p.mark_upper) == (64, 4500, 63, 0)                    # ref: include/Utility.hpp:52-53
    assert F(p.ang_res_y) == F(26.9) / F(63) and F(p.ang_bottom) == F(15.1)                                 # ref: :55-56
    assert (F(p.mount_deg), F(p.tol_deg), F(p.min_range)) == (F(0), F(2.5), F(0.1))                        # ref: :58, src/Utility.cpp:529, :484
    assert capi.load().tsdf_scan_ground_params_default(None) == -1


def test_struct_layout_matches_c(tmp_path):
    fields = [f for f, _ in capi.ScanGroundParams._fields_]
    body = "\n".join(f'printf("{f} %zu\\n", offsetof(tsdf_scan_ground_params, {f}));' for f in fields)
    prog = tmp_path / "layout.c"
    prog.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "tsdf_hip.h"\n'
                    'int main(void){printf("size %zu\\n", sizeof(tsdf_scan_ground_params));\n' + body + "\nreturn 0;}\n")
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(prog), "-o", str(exe)])
    got = dict(line.split() for line in subprocess.check_output([str(exe)]).decode().splitlines())
    assert int(got["size"]) == C.sizeof(capi.ScanGroundParams)
    for f in fields:
        assert int(got[f]) == getattr(capi.ScanGroundParams, f).offset, f


@pytest.mark.parametrize("p", [spec.DEFAULT, spec.HDL64E, cases.P2, cases.P5, cases.P8, cases.PW], ids=lambda p: f"{p.n_rings}x{p.n_columns}")
def test_library_tables_are_the_rule_s(p):
    """The library's tables against NumPy's: the quadrants' runs are the same; the values agree to an ulp (two libms) and, on this
    build, to the bit."""
    a, b = spec.tables(p), spec.tables_numpy(p)
    assert np.array_equal(a["first"], b["first"]) and np.array_equal(a["len"], b["len"]) and a["len"].sum() == p.n_columns
    for k in ("T", "C", "S"):
        assert a[k].shape == b[k].shape
        assert np.all(np.abs(a[k].astype(np.float64) - b[k]) <= np.spacing(np.abs(b[k])) + 1e-45), k
    assert np.all(np.diff(a["T"]) >= 0)
    assert np.array_equal(spec.quadrant(a["C"], a["S"]), spec.quadrant(b["C"], b["S"]))


def test_every_invalid_parameter_is_refused():
    lib = capi.load()
    big = np.zeros(1 << 15, F)
    out = np.zeros(8, np.int32)
    good = capi.scan_ground_params_default()
    args = (big.ctypes.data, big.ctypes.data, big.ctypes.data, big.ctypes.data, out.ctypes.data, out.ctypes.data)
    assert lib.tsdf_scan_ground_tables(C.addressof(good), *args) == 0
    for bad in cases.INVALID:
        p = capi.scan_ground_params_default()
        for k, v in bad.items():
            setattr(p, k, v)
        assert lib.tsdf_scan_ground_tables(C.addressof(p), *args) == -1 and b"ground_params" in lib.tsdf_last_error(), bad
    for lim in (dict(n_rings=2, ground_rings=1, ang_res_y=1.0), dict(n_rings=128, ang_res_y=0.5), dict(n_columns=4), dict(n_columns=16384),
                dict(ground_rings=0), dict(tol_deg=0.0), dict(min_range=0.0), dict(mount_deg=87.0, tol_deg=2.5)):
        p = capi.scan_ground_params_default()
        for k, v in lim.items():
            setattr(p, k, v)
        assert lib.tsdf_scan_ground_tables(C.addressof(p), *args) == 0, lim
    assert lib.tsdf_scan_ground_tables(None, *args) == -1


def test_table_builder_under_the_sanitizers(tmp_path):
    """csrc/scan_ground_tables.h behind tests/scan_ground_tables_check.cpp, built with ASan + UBSan and run as a child process."""
    assert shutil.which("g++"), "the table check needs g++"
    exe = tmp_path / "scan_ground_tables_check"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "semantic_slam_amd", "csrc"), "-o", str(exe),
                           os.path.join(ROOT, "tests", "scan_ground_tables_check.cpp")])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    p = subprocess.run([str(exe)], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    out = p.stdout.decode()
    assert p.returncode == 0 and not p.stderr and "FAILED" not in out, f"rc {p.returncode}\n{out[-4000:]}\n{p.stderr.decode()[-4000:]}"
    assert out.strip().splitlines()[-1].startswith("checked ")


# ---- the rule against the reference's formula -----------------------------------------------------------------------------
MARGIN = 1e-3            # of a cell: float32 products put a border off by about 4e-5 of a 0.08 degree cell


def against_reference(points, p):
    """(share of points nearer than MARGIN to a border, disagreements outside the margin, disagreements inside it)."""
    c = spec.cells(points, p, spec.tables(p))
    ring_f, col_f, ring, col = spec.reference_cells(points, p)
    near = (np.abs(ring_f - np.round(ring_f)) < MARGIN) | (np.abs(col_f + 0.5 - np.round(col_f + 0.5)) < MARGIN)
    ref_ok = (ring >= 0) & (ring < p.n_rings)
    x, y, z = (np.asarray(points, np.float64)[:, i] for i in range(3))
    ref_ok &= np.sqrt(x * x + y * y + z * z) >= float(p.min_range)
    same = np.where(ref_ok, (c["ring"] == ring) & (c["col"] == col), c["ring"] == -1)
    return float(np.mean(near)), int(np.count_nonzero(~same & ~near)), int(np.count_nonzero(~same & near))


@pytest.mark.parametrize("p", [spec.DEFAULT, cases.P5], ids=["64x4500", "5x36"])
def test_cells_are_the_reference_formula_s(p):
    pts = np.zeros((20000, 4), F)
    pts[:, :3] = np.random.default_rng(11).normal(0.0, 10.0, (20000, 3))
    share, outside, inside = against_reference(pts, p)
    print(f"{p.n_rings} x {p.n_columns}: {100 * share:.2f} % within {MARGIN} of a border; disagreements {outside} outside, {inside} inside")
    assert share < 0.01
    assert outside == 0


def test_cells_of_the_street_scan_are_the_reference_formula_s():
    pts = scan_cases.calibration_case()["points"]
    for p in (spec.DEFAULT, spec.HDL64E):
        share, outside, inside = against_reference(pts, p)
        print(f"kitti_scan, bottom {float(p.ang_bottom):.2f}: {100 * share:.2f} % near a border; disagreements {outside} outside, {inside} inside")
        assert outside == 0


def test_level_test_is_the_reference_angle_test():
    """dz >= tlo hd && dz <= thi hd against |atan2(dz, hd) deg - mount| <= tol in float64, on the street scan's and on random
    cells' pairs that are further than 1e-3 degrees from either limit."""
    for c in (cases.kitti_marks("hdl64e"), cases.kitti_marks("default"), cases.random_case(3), cases.random_case(16)):
        p, pts, w = c["params"], c["points"].astype(np.float64), c["want"]
        pair = spec.pair_states(c["points"], w["winner"].astype(np.int64), p, c["tab"])
        lo, hi = w["winner"][:-1], w["winner"][1:]
        both = (lo >= 0) & (hi >= 0)
        d = pts[np.where(both, hi, 0)] - pts[np.where(both, lo, 0)]
        angle = np.degrees(np.arctan2(d[..., 2], np.hypot(d[..., 0], d[..., 1])))
        off = np.abs(angle - float(p.mount_deg))
        clear = both & (np.abs(off - float(p.tol_deg)) > 1e-3)
        assert np.count_nonzero(clear) > 100
        assert np.array_equal(pair[clear] == 1, off[clear] <= float(p.tol_deg))


# ---- the named cases ------------------------------------------------------------------------------------------------------
def test_every_case_is_there():
    names = [c["name"] for c in cases.small_cases()]
    assert len(names) == len(set(names))
    for part in ("ring_borders_exact", "column_borders_exact", "quadrants_and_axes", "straddling_cells_k0", "wrap_cells", "no_cell",
                 "later_wins_two_level", "later_wins_two_steep", "later_wins_three", "slope_at_thi_exactly", "slope_at_thi_one_ulp_over",
                 "slope_at_tlo_exactly", "slope_at_tlo_one_ulp_over", "upper_cell_empty", "stacked_points_hd_zero", "ground_then_wall",
                 "ground_then_wall_mark_upper", "ground_rings_0", "ground_rings_1_mark_upper", "count_0_2x4", "count_1_5x36", "count_255_8x64",
                 "count_256_5x36", "count_257_64x4500", "count_4097_5x36", "count_4097_2x4"):
        assert part in names, part
    assert cases.identical_points_pair()[0, 0] == 1                     # hd == dz == 0 is level


def test_scalar_restatement_equals_the_vectorised_one_on_every_small_case():
    for c in cases.small_cases():
        got = spec.mark_scalar(c["points"], c["params"], c["tab"])
        for k in ("flags", "state", "winner", "counts"):
            assert np.array_equal(got[k], c["want"][k]), (c["name"], k)


@pytest.mark.parametrize("seed", [0, 4, 9, 14])
def test_scalar_restatement_on_random_cases(seed):
    c = cases.random_case(seed)
    got = spec.mark_scalar(c["points"], c["params"], c["tab"])
    for k in ("flags", "state", "winner", "counts"):
        assert np.array_equal(got[k], c["want"][k]), (c["name"], k)


def test_scalar_restatement_on_a_part_of_the_street_scan():
    """Every 40th azimuth of the scan (64 points each) under the sensor's parameters, the upper cell marked."""
    pts = scan_cases.calibration_case()["points"].reshape(-1, 64, 4)[::40].reshape(-1, 4)
    p = spec.HDL64E._replace(mark_upper=1)
    a, b = spec.mark(pts, p), spec.mark_scalar(pts, p)
    for k in ("flags", "state", "winner", "counts"):
        assert np.array_equal(a[k], b[k]), k
    assert a["counts"][3] > 2000


# ---- what it finds --------------------------------------------------------------------------------------------------------
def test_the_reference_literals_miss_the_sensor():
    """The reference's rings cover -15.1 ... +11.8 degrees, an HDL-64E fires +2 ... -24.8: 42 780 of the street scan's 119 040 points
    have no cell and about half of its ground returns are marked."""
    c = cases.kitti_marks("default")
    f, gt = c["want"]["flags"], cases.is_ground_truth(c["points"])
    assert len(f) == 119040 and np.count_nonzero(f == 2) == 42780
    assert 0.50 < np.mean(f[gt] == 1) < 0.54


def test_the_street_scan_s_ground_is_found():
    c = cases.kitti_marks("hdl64e")
    f, gt = c["want"]["flags"], cases.is_ground_truth(c["points"])
    n_gt, n_other = int(np.count_nonzero(gt)), int(np.count_nonzero(~gt))
    hit, false = int(np.count_nonzero(f[gt] == 1)), int(np.count_nonzero(f[~gt] == 1))
    print(f"mark_upper 0: {hit} of {n_gt} ground returns marked, {false} of {n_other} others")
    assert not np.any(f == 2)
    assert hit >= 0.95 * n_gt
    assert false <= 0.001 * n_other
    c = cases.kitti_marks("hdl64e_upper")
    f = c["want"]["flags"]
    hit, false = int(np.count_nonzero(f[gt] == 1)), int(np.count_nonzero(f[~gt] == 1))
    print(f"mark_upper 1: {hit} of {n_gt} ground returns marked, {false} of {n_other} others")
    assert hit == n_gt
    assert false <= 0.05 * n_other


def ground_band_voxels(oracle, depth):
    """Voxels of kitti_scene() that the oracle fuses into the band |tsdf| < 1 within one truncation distance of the ground plane,
    those in the back wall's own band left out."""
    scene = scan_cases.kitti_scene()
    cal = scan_cases.golden_calibration()
    pose = scene.pose(0, n=16, max_yaw_deg=5.0)
    K = scan_cases.calibration_case()["K"]
    trunc = float(F(scene.vs) * F(5))
    t, w = oracle.init_grid(scene.dims)
    oracle.integrate(K, oracle.cam2base(synth.identity_pose(), pose), depth, scene.dims, scene.origin.astype(F), scene.vs, trunc, t, w,
                     max_depth=80.0)
    velo2cam = np.eye(4)
    velo2cam[:3, :3], velo2cam[:3, 3] = cal["R_velo"], cal["t_velo"]
    T = np.asarray(pose, np.float64).reshape(4, 4) @ velo2cam                    # sensor to base
    normal, on_plane = T[:3, 2], T[:3, :3] @ np.array([0.0, 0.0, -1.73]) + T[:3, 3]
    dx, dy, dz = scene.dims
    z, y, x = np.meshgrid(np.arange(dz), np.arange(dy), np.arange(dx), indexing="ij")
    X = np.stack([x, y, z], axis=-1).reshape(-1, 3) * scene.vs + scene.origin
    near_ground = np.abs((X - on_plane) @ normal) <= trunc
    clear_of_wall = X[:, 2] < scene.wall_z - 2 * trunc
    band = (w > 0) & (np.abs(t) < 1)
    return int(np.count_nonzero(band & near_ground & clear_of_wall)), int(np.count_nonzero(band))


def test_a_fused_volume_loses_the_road(oracle):
    s = scan_cases.calibration_case()
    filled = scan_fill_cases.kitti_case()["filled"]                                   # N15: the whole scan, filled
    flags = cases.kitti_marks("hdl64e_upper")["want"]["flags"]
    assert not np.any(flags[cases.is_ground_truth(s["points"])] != 1)                # no ground return survives
    kept = spec.select(s["points"], flags, spec.DROP_GROUND)
    dropped, _, _ = scan_fill_spec.fill(scan_spec.scan_depth(kept, s["velo2img"], s["K"], s["H"], s["W"]), *scan_fill_spec.DEFAULT)
    with_road, band_all = ground_band_voxels(oracle, filled)
    without, band_dropped = ground_band_voxels(oracle, dropped)
    print(f"ground-band voxels: {with_road} with the ground returns, {without} without (band {band_all} and {band_dropped})")
    assert with_road > 1000
    assert without * 10 <= with_road
    assert band_dropped > 0.3 * (band_all - with_road)                                # what stands on the road is still fused
