"""The scan tracking rule on the CPU (tests/scan_track_spec.py restates csrc/tsdf_scan_track.hip.h; tests/scan_track_cases.py
builds the cases): none of the cases tests/test_gpu_scan_track.py holds the device to is vacuous -- every named case reaches
the branch it is named for --, a second, scalar statement of the per-point rule agrees with the vectorised one bit for bit, the
restatement converges inside the basin and is lost outside it, and the host-only entry points (tsdf_scan_pose,
tsdf_scan_track_params_default) answer as the header says."""
import ctypes as C
import os

import numpy as np
import pytest

import scan_track_cases as sc
import scan_track_spec as sts
from semantic_slam_amd import capi

f32 = np.float32
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "kitti_2011_09_30_calib.npz")


# ------------------------------------------------------------------------------------------------------------------------
# the named cases
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", sc.named_cases(), ids=repr)
def test_named_case_reaches_its_branch(case):
    info = {}
    terms = case.terms(0, info)
    assert len(terms) == len(info["idx"]) == info["selected"] - sum(info["rejected"].values())
    if not case.special:                                           # a count case: what it says about its pairs
        assert len(terms) > 0 or len(case.points) == 0
        return
    special = np.asarray(case.special)
    assert np.all(special % 4 == 0), "selected at every level"
    # the hand-placed points alone, under the same parameters: every one of them ends at the gate the case is named for
    alone = sc.SystemCase(case.name, case.points[special], P=case.P, flags=None if case.flags is None else case.flags[special])
    i = {}
    alone.terms(0, i)
    if case.gate is None:
        assert i["rejected"] == dict.fromkeys(sts.GATES, 0) and np.isin(special, info["idx"]).all(), (case, i["rejected"])
    else:
        want = dict.fromkeys(sts.GATES, 0)
        want[case.gate] = len(special)
        assert i["rejected"] == want and not np.isin(special, info["idx"]).any(), (case, i["rejected"])
    assert len(terms) >= 40, "the other points of the case make pairs"


def test_the_thresholds_are_met_exactly():
    """What makes "exactly at" exact: the squares of the ranges, the grid coordinates 0 and dim - 1, F and r of the point on
    the prepared voxel."""
    cases = {c.name: c for c in sc.named_cases()}
    P = sc.exact_params()
    assert float(P["min_range_m"] * P["min_range_m"]) == 0.25 and float(P["max_range_m"] * P["max_range_m"]) == 2.25
    for name, want in (("range exactly at min_range_m", 0.25), ("range exactly at max_range_m", 2.25)):
        p = cases[name].points[list(cases[name].special), :3]
        assert np.all((p[:, 0] * p[:, 0] + p[:, 1] * p[:, 1]) + p[:, 2] * p[:, 2] == f32(want)), name
    outside = cases["range one ulp outside"]
    p = outside.points[list(outside.special), :3]
    d2 = (p[:, 0] * p[:, 0] + p[:, 1] * p[:, 1]) + p[:, 2] * p[:, 2]
    # a coordinate one ulp off moves the square by two ulps of the coordinate: the nearest squares the other side of the rule
    assert f32(0.25) * f32(1 - 2.0 ** -22) < d2[0] < f32(0.25) and f32(2.25) < d2[1] <= np.nextafter(f32(2.25), f32(3))
    _, _, grid = sc.exact_world()
    org, vs = np.asarray(grid[1], f32), f32(grid[2])
    for name, want in (("g exactly 0", 0.0), ("g exactly dim - 1", 47.0)):
        p = cases[name].points[list(cases[name].special), :3]
        g = (p - org) / vs
        assert [float(g[k, k]) for k in range(3)] == [want] * 3, name
    on, over = cases["|r| == resid_thresh"], cases["|r| the next float after resid_thresh"]
    assert on.P["resid_thresh"] == over.P["resid_thresh"] == f32(0.5) * f32(grid[3])
    r_on = np.sqrt(on.terms(0)[np.flatnonzero(np.isin(_idx(on), on.special))[0], 27])
    assert f32(r_on) == on.P["resid_thresh"]
    # the same point under the default resid_thresh is a pair whose r is the next float
    relaxed = sc.SystemCase("relaxed", over.points, P=sc.exact_params())
    r_over = np.sqrt(relaxed.terms(0).astype(np.float64)[np.flatnonzero(np.isin(_idx(relaxed), over.special))[0], 27])
    assert f32(r_over) > over.P["resid_thresh"] and f32(r_over) <= np.nextafter(over.P["resid_thresh"], f32(1)) * f32(1.0000002)


def _idx(case):
    i = {}
    case.terms(0, i)
    return i["idx"]


@pytest.mark.parametrize("level", sc.LEVELS)
@pytest.mark.parametrize("case", sc.named_cases(), ids=repr)
def test_scalar_statement_agrees_bit_for_bit(case, level):
    a, b = {}, {}
    vec, sca = case.terms(level, a), case.terms(level, b, scalar=True)
    assert vec.shape == sca.shape and vec.tobytes() == sca.tobytes(), case
    assert np.array_equal(a["idx"], b["idx"]) and a["rejected"] == b["rejected"]


def test_counts_and_strides():
    for n in sc.COUNTS:
        c = sc.count_case(n)
        for level in sc.LEVELS:
            i = {}
            c.terms(level, i)
            assert i["selected"] == -(-n // (1 << level))
            assert np.all(i["idx"] % (1 << level) == 0)
    big = sc.count_case(65601)
    i = {}
    big.terms(0, i)
    assert (i["idx"] >= sc.MAX_BLOCKS * 256).sum() == 65, "pairs in the lanes the grid-stride loop wraps to"
    odd = [c for c in sc.named_cases() if c.name.startswith("n_points not a multiple")][0]
    assert len(odd.points) % 2 == 1 and len(odd.points) % 4 == 3
    for level in (1, 2):
        i = {}
        odd.terms(level, i)
        assert i["selected"] == -(-len(odd.points) // (1 << level)) and i["idx"].max() == (len(odd.points) - 1) // (1 << level) * (1 << level)


def test_scalar_statement_on_the_corner_scan():
    cfg, vol, grid = sc.corner_world()
    pts, truth = sc.corner_scan()
    guess = sc.convergence_cases()[2].guess
    M = sts.start_pose(grid, guess)
    Rm, tm = M[:, :3].astype(f32), M[:, 3].astype(f32)
    P = sc.corner_params()
    a, b = {}, {}
    vec = sts.pair_terms(vol, grid, pts[::3], None, Rm, tm, 0, P, a)
    sca = sts.pair_terms_scalar(vol, grid, pts[::3], None, Rm, tm, 0, P, b)
    assert len(vec) > 300 and vec.tobytes() == sca.tobytes() and a["rejected"] == b["rejected"]
    assert a["rejected"]["box"] > 0 and a["rejected"]["corner"] > 0 and a["rejected"]["range"] > 0


# ------------------------------------------------------------------------------------------------------------------------
# whole runs
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", range(len(sc.INSIDE)), ids=[n for n, _, _, _ in sc.INSIDE])
def test_convergence_inside_the_basin(k):
    case = sc.convergence_cases()[k]
    _, truth = sc.corner_scan()
    want = case.want()
    r0, t0 = sts.pose_error(case.guess, truth)
    r1, t1 = sts.pose_error(want["velo2world"], truth)
    print(f"{case}: guess {r0:.4f} deg {1e3 * t0:.2f} mm -> {r1:.4f} deg {1e3 * t1:.2f} mm from the truth; status {want['status']}, "
          f"iters_run {want['iters_run']}, {want['pairs']} pairs of {len(case.points)} points, rmse {1e3 * want['rmse']:.3f} mm")
    assert want["status"] == 0
    # nearer than the guess in the part the guess displaced; a part the guess left exact (a pure translation has no rotation
    # error to come nearer than) must end below the smallest displacement any of the guesses starts with in that part
    least_deg = min(d for _, d, _, _ in sc.INSIDE if d > 0)
    least_m = min(m for _, _, m, _ in sc.INSIDE if m > 0)
    assert r1 < (r0 if r0 > 0.0 else least_deg)
    assert t1 < (t0 if t0 > 0.0 else least_m)
    assert sc.preconditions(want["history"], case.P) == []


def test_outside_the_basin_is_lost_or_no_nearer():
    _, truth = sc.corner_scan()
    case = sc.lost_cases()[0]
    want = case.want()
    r0, t0 = sts.pose_error(case.guess, truth)
    r1, t1 = sts.pose_error(want["velo2world"], truth)
    print(f"{case}: status {want['status']}, {want['pairs']} pairs; {1e3 * t0:.1f} mm -> {1e3 * t1:.1f} mm from the truth")
    assert want["status"] == 2 or t1 >= t0


@pytest.mark.parametrize("k", range(1, 4))
def test_lost_runs_return_the_guess(k):
    case = sc.lost_cases()[k]
    want = case.want()
    assert want["status"] == 2 and want["lost"] and want["iters_run"] == [0, 0, 1], case
    assert want["velo2world"].tobytes() == case.guess.tobytes()
    assert want["pairs"] == 0 and want["rmse"] == 0.0


def test_last_row_of_the_guess_is_not_read_but_returned():
    cfg, vol, grid = sc.corner_world()
    _, truth = sc.corner_scan()
    odd = truth.copy()
    odd[12:] = [3.0, np.nan, -1.0, 7.0]
    assert np.array_equal(sts.start_pose(grid, odd), sts.start_pose(grid, truth))
    lost = sts.track(vol, grid, np.zeros((0, 4), f32), None, sc.corner_params(), odd)
    assert lost["status"] == 2 and lost["velo2world"].tobytes() == odd.tobytes()


# ------------------------------------------------------------------------------------------------------------------------
# the host-only entry points
# ------------------------------------------------------------------------------------------------------------------------
def test_scan_pose_on_the_golden_calibration():
    cal = np.load(GOLDEN)
    got = capi.scan_pose(cal["R_rect"], cal["R_velo"], cal["t_velo"])
    want = sts.scan_pose(cal["R_rect"], cal["R_velo"], cal["t_velo"])
    assert got.dtype == np.float32 and got.tobytes() == want.tobytes()
    assert got[3].tolist() == [0.0, 0.0, 0.0, 1.0]
    # the first three rows of velo2img are P_rect times it
    v2i = capi.scan_projection(cal["P_rect"], cal["R_rect"], cal["R_velo"], cal["t_velo"])
    assert np.allclose(v2i, cal["P_rect"].astype(np.float64) @ got.astype(np.float64), rtol=1e-5, atol=1e-3)


def test_scan_pose_refusals():
    lib = capi.load()
    a, t, out = np.eye(3, dtype=f32).ravel(), np.zeros(3, f32), np.full(16, 7.0, f32)
    args = [a.ctypes.data, a.ctypes.data, t.ctypes.data, out.ctypes.data]
    for k in range(4):
        bad = list(args)
        bad[k] = None
        assert lib.tsdf_scan_pose(*bad) == -1 and b"tsdf_scan_pose" in lib.tsdf_last_error() and b"NULL" in lib.tsdf_last_error()
    assert np.all(out == 7.0)
    assert lib.tsdf_scan_pose(*args) == 0 and np.array_equal(out, np.eye(4, dtype=f32).ravel())


def test_params_default():
    cfg = capi.make_config((48, 48, 48), 0.1, np.zeros(3, f32))
    p = capi.scan_track_params_default(cfg)
    assert p.weight_thresh == f32(0.9) and p.resid_thresh == f32(cfg.trunc_margin) == f32(0.1) * f32(5)
    assert (p.min_range_m, p.max_range_m) == (2.5, 80.0)
    assert (p.n_levels, list(p.iters), p.min_pairs, p.drop_flag) == (3, [10, 5, 4], 300, -1)
    assert p.eps_rot == f32(1e-5) and p.eps_trans == f32(1e-5)
    lib = capi.load()
    out = capi.ScanTrackParams()
    out.n_levels = 77
    assert lib.tsdf_scan_track_params_default(None, C.byref(out)) == -1 and b"tsdf_scan_track_params_default" in lib.tsdf_last_error()
    assert lib.tsdf_scan_track_params_default(C.byref(cfg), None) == -1 and b"NULL" in lib.tsdf_last_error()
    assert out.n_levels == 77
    spec = sts.from_ctypes(p)
    back = sts.to_ctypes(spec)
    assert bytes(back) == bytes(p)


def test_struct_layout_matches_c(tmp_path):
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    lines = []
    for struct, mirror in (("tsdf_scan_track_params", capi.ScanTrackParams), ("tsdf_scan_track_result", capi.ScanTrackResult)):
        lines.append(f'printf("{struct} %zu\\n", sizeof({struct}));')
        lines += [f'printf("{struct}.{f} %zu\\n", offsetof({struct}, {f}));' for f, _ in mirror._fields_]
    prog = tmp_path / "layout.c"
    prog.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "tsdf_hip.h"\nint main(void){\n' + "\n".join(lines) + "\nreturn 0;}\n")
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(root, "include"), str(prog), "-o", str(exe)])
    got = dict(line.split() for line in subprocess.check_output([str(exe)]).decode().splitlines())
    for struct, mirror in (("tsdf_scan_track_params", capi.ScanTrackParams), ("tsdf_scan_track_result", capi.ScanTrackResult)):
        assert int(got[struct]) == C.sizeof(mirror)
        for f, _ in mirror._fields_:
            assert int(got[f"{struct}.{f}"]) == getattr(mirror, f).offset, (struct, f)
