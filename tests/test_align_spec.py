"""The registration rule (csrc/tsdf_align.hip.h) in its NumPy restatement tests/align_spec.py, without a GPU: the C structs,
the defaults and tsdf_fuse_pose_default, the identities of the rule, convergence on volumes fused from depth frames against
the known motion, and the conditions under which the cases of tests/test_gpu_align.py (tests/align_cases.py) mean anything.

Convergence, measured with the restatement on synth.TrackScene fused through the CPU oracle into a (64, 48, 40) destination at
4 mm (four views) and a (52, 42, 34) source at 5 mm (eight views), default parameters, the source's base2world off by a seeded
motion about the scene's centre (errors against the true motion; translation at the scene's centre):

    start            ended      iterations (level 1 + level 0)   final error            pairs    rmse
    1 deg /   3 mm   converged  5 + 7                            0.196 deg / 0.497 mm   30 356   0.0804
    2 deg /   6 mm   converged  6 + 7                            0.196 deg / 0.497 mm   30 356   0.0804
    4 deg /  10 mm   converged  7 + 7                            0.196 deg / 0.497 mm   30 356   0.0804
    8 deg /  20 mm   converged  9 + 7                            0.196 deg / 0.497 mm   30 356   0.0804
    30 deg / 100 mm  lost       1 + 0                            (the start's own bits) 273      0.715

Every run inside the basin ends at the same minimum: what is left is not the solver's error but the distance between the
minimum of the SDF difference of two volumes fused from different views at different voxel sizes and the true motion.  The
assertions below allow twice the recorded final error: the margin covers the spread across seeds of the perturbation and of
the views, not a weaker solver."""
import ctypes as C
import os
import subprocess

import numpy as np

import align_cases as ac
import align_spec as asp
import fuse_spec as fs
from semantic_slam_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
# the recorded final errors of the table (degrees, metres), pairs and rmse
RECORDED = {"rot_deg": 0.1964, "trans_m": 0.4975e-3, "pairs": 30356, "rmse": 0.0804}


def test_struct_layouts_and_defaults(tmp_path):
    p = capi.align_params_default(capi.default_config())
    assert (f32(p.weight_thresh), f32(p.resid_thresh), p.n_levels, list(p.iters), p.min_pairs) == (f32(0.9), f32(1.0), 2, [10, 10, 0], 300)
    assert f32(p.eps_rot) == f32(1e-5) and f32(p.eps_trans) == f32(1e-5)
    assert asp.from_ctypes(p) == asp.params()
    lib = capi.load()
    assert lib.tsdf_align_params_default(None, C.byref(p)) == -1 and b"tsdf_align_params_default" in lib.tsdf_last_error()
    mirrors = {"tsdf_align_params": capi.AlignParams, "tsdf_align_result": capi.AlignResult}
    body = ""
    for name, cls in mirrors.items():
        body += f'printf("{name} size %zu\\n", sizeof({name}));\n'
        body += "".join(f'printf("{name} {f} %zu\\n", offsetof({name}, {f}));\n' for f, _ in cls._fields_)
    prog = tmp_path / "layout.c"
    prog.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "tsdf_hip.h"\nint main(void){\n' + body + "return 0;}\n")
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(prog), "-o", str(exe)])
    got = {tuple(line.split()[:2]): int(line.split()[2]) for line in subprocess.check_output([str(exe)]).decode().splitlines()}
    for name, cls in mirrors.items():
        assert got[(name, "size")] == C.sizeof(cls), name
        for f, _ in cls._fields_:
            assert got[(name, f)] == getattr(cls, f).offset, (name, f)


def test_fuse_pose_default_is_the_pose_the_merge_composes():
    lib = capi.load()
    seen = 0
    for dims in ac.DST_SHAPES:
        for pose in range(ac.N_POSES):
            for a, b in (ac.configs(dims, pose), ac.configs(dims, pose)[::-1]):
                got = capi.fuse_pose_default(a, b)
                want = fs.relative_pose(np.array(b.base2world, f32), np.array(a.base2world, f32))
                assert got.tobytes() == np.asarray(want, f32).tobytes(), (dims, pose)
                seen += 1
    assert seen == 18
    singular = ac.configs(ac.BIG, 0)[1]
    singular.base2world[:] = [0.0] * 16                      # the all-zero inverse, as everywhere else
    assert not capi.fuse_pose_default(ac.configs(ac.BIG, 0)[0], singular).any()
    out = np.zeros(16, f32)
    assert lib.tsdf_fuse_pose_default(None, C.byref(singular), out.ctypes.data) == -1 and b"tsdf_fuse_pose_default" in lib.tsdf_last_error()
    assert lib.tsdf_fuse_pose_default(C.byref(singular), C.byref(singular), None) == -1


def test_fuse_at_the_default_pose_is_fuse():
    dcfg, scfg, (dt, dw, st, sw) = ac.states(ac.DST_SHAPES[0], 2, "edges")
    dg, sg = fs.grid_of(dcfg), fs.grid_of(scfg)
    want = fs.fuse(dt, dw, dg, st, sw, sg)
    got = asp.fuse_at(dt, dw, dg, st, sw, sg, asp.pose_default((dg, sg)))
    assert got[2] == want[2] and not fs.differs(got[0], want[0]).any() and not fs.differs(got[1], want[1]).any()
    other = asp.fuse_at(dt, dw, dg, st, sw, sg, ac.moved(asp.pose_default((dg, sg)), ac.centre_of(dcfg), 3.0, 0.01, 1))
    assert other[2] != want[2]
    assert fs.fuse(dt, dw, dg, st, sw, sg)[2] == want[2]     # relative_pose was put back


def test_identical_grids_with_identical_content_have_no_residual():
    """g_i is the integer x_i (a power-of-two voxel size), f = 0, F = the voxel's own value: r = 0 in every pair, so b = 0 and
    sum r^2 = 0, while the gradient -- there is no collapse onto the lattice -- is not zero and pairs exist."""
    _, scfg = ac.exact_grids()
    t, w = ac.exact_source()
    g = fs.grid_of(scfg)
    for level in ac.LEVELS:
        info = {}
        sums, _ = asp.system((t, w), (t, w), (g, g), asp.start_pose((g, g)), level, asp.params(n_levels=3), info)
        assert sums[28] > 0.5 * info["lattice"] and not sums[21:28].any(), (level, sums[21:29])
        assert np.all(sums[[0, 6, 11, 15, 18, 20]] > 0)      # the diagonal of J^T J
        assert (info["rejected"]["box"] > 0) == (level == 0)  # the last voxel of an axis has no upper corner; s | dim above


def test_the_first_step_reduces_a_known_small_motion():
    dcfg, _, arrays, truth = ac.run_world()
    cfg, _ = ac.perturbed_source(*ac.MAGNITUDES[0])
    grids = (fs.grid_of(dcfg), fs.grid_of(cfg))
    c = ac.centre_of(dcfg)
    e0 = asp.motion_error(asp.pose_default(grids), truth, c)
    r = asp.align(arrays[:2], arrays[2:], grids, asp.params(n_levels=1, iters=(1, 0, 0)))
    e1 = asp.motion_error(r["dst2src"], truth, c)
    print(f"start {e0[0]:.3f} deg {1e3 * e0[1]:.2f} mm, after one step {e1[0]:.3f} deg {1e3 * e1[1]:.2f} mm")
    assert r["status"] == 1 and r["iters_run"] == [1, 0, 0]
    assert e1[0] < 0.5 * e0[0] and e1[1] < 0.5 * e0[1]


def test_convergence_on_fused_volumes():
    dcfg, _, arrays, truth = ac.run_world()
    c = ac.centre_of(dcfg)
    for deg, metres, seed in ac.MAGNITUDES:
        cfg, _ = ac.perturbed_source(deg, metres, seed)
        grids = (fs.grid_of(dcfg), fs.grid_of(cfg))
        start = asp.pose_default(grids)
        hist = []
        r = asp.align(arrays[:2], arrays[2:], grids, asp.params(), None, hist)
        e0, e1 = asp.motion_error(start, truth, c), asp.motion_error(r["dst2src"], truth, c)
        ratio0 = ac.band_ratio(asp.fuse_at(arrays[0], arrays[1], grids[0], arrays[2], arrays[3], grids[1], start, write=0)[2])
        ratio1 = ac.band_ratio(asp.fuse_at(arrays[0], arrays[1], grids[0], arrays[2], arrays[3], grids[1], r["dst2src"], write=0)[2])
        print(f"start {e0[0]:.3f} deg {1e3 * e0[1]:.2f} mm: status {r['status']}, iterations {r['iters_run']}, final {e1[0]:.4f} deg "
              f"{1e3 * e1[1]:.4f} mm, pairs {r['pairs']}, rmse {r['rmse']:.4f}, agree_band / both_band {ratio0:.3f} -> {ratio1:.3f}")
        assert abs(e0[0] - deg) < 0.01 * deg and abs(e0[1] - metres) < 0.01 * metres
        if (deg, metres, seed) in ac.INSIDE:
            assert r["status"] == 0 and sum(r["iters_run"]) <= 20
            assert e1[0] <= 2 * RECORDED["rot_deg"] and e1[1] <= 2 * RECORDED["trans_m"], (deg, e1)
            assert r["pairs"] >= 0.10 * hist[-1]["lattice"] and r["rmse"] <= 2 * RECORDED["rmse"]
            assert ratio1 > ratio0
        else:                                                 # outside the basin: lost, the start's own bits
            assert r["status"] == 2 and r["lost"] and r["dst2src"].tobytes() == start.tobytes()
            assert ratio1 == ratio0 < 0.5


def test_the_gpu_system_cases_are_not_vacuous():
    """Every parity case: pairs >= 10 % of the lattice; every rejection class non-empty (at ratio 0.75 a source fused by
    Integrate cannot leave the band -- align_cases' docstring -- and that class must then be empty); no computed comparison
    within one float32 spacing of its threshold."""
    keys = ac.parity_keys()
    assert len(keys) == 54
    ratios = set()
    for key in keys:
        c = ac.parity_case(*key)
        rej, n = c.info["rejected"], len(c.terms)
        assert n >= 0.10 * c.info["lattice"], (c, n, c.info["lattice"])
        ratios.add(float(f32(c.scfg.trunc_margin) / f32(c.dcfg.trunc_margin)))
        for gate in ("candidate", "box", "corner", "band", "resid"):
            if gate == "band" and key[2] == "surf" and key[1] == 1:
                assert rej[gate] == 0, (c, rej)
            else:
                assert rej[gate] > 0, (c, gate, rej)
        if key[2] == "edges" and key[3] == 0:                # an infinite or NaN corner: a sample that is not finite
            assert rej["finite"] > 0, (c, rej)
        assert not any(c.info["near"].values()), (c, c.info["near"])
    assert {round(r, 5) for r in ratios} == {0.75, 1.25}
    assert ac.device_lanes(ac.BIG, 0)[2] > ac.MAX_BLOCKS * 256        # more than one trip of the grid-stride loop
    assert any(d[0] % ac.TILE_X and d[1] % ac.TILE_Y for d in ac.DST_SHAPES)          # partial tiles on both axes


def test_the_exact_families_have_their_pair_counts():
    for n in ac.EXACT_COUNTS:
        c = ac.reduction_case(n)
        assert len(c.terms) == n == c.info["candidates"], (n, len(c.terms))
    c, first = ac.last_trip_case()
    lane, blocks, lanes = ac.device_lanes(ac.BIG, 0)
    assert len(c.terms) == c.info["candidates"] >= 8
    assert lane[c.info["idx"]].min() >= first and first >= blocks * 256 and lanes - first <= 256
    single = ac.picked_case("one pair", ac.interior_points()[[777]])
    assert len(single.terms) == 1 and single.terms[0, 28] == 1.0 and np.all(single.terms[0, :21][[0, 6, 11, 15, 18, 20]] > 0)


def test_the_gpu_runs_keep_clear_of_the_thresholds():
    cases = ac.state_machine_cases()
    statuses = set()
    for c in cases:
        w = c.want()
        assert ac.preconditions(w["history"], c.P) == [], (c, ac.preconditions(w["history"], c.P))
        statuses.add(w["status"])
    assert statuses == {0, 1, 2}
    by_name = {c.name: c.want() for c in cases}
    a, b = [by_name[n] for n in by_name if n.startswith("min_pairs")]
    assert a["status"] != 2 and b["status"] == 2 and b["iters_run"] == [0, 0, 1]
    skipped = by_name["n_levels 3 iters (0, 4, 0) eps 1e-05"]
    assert skipped["iters_run"][0] == 0 and skipped["iters_run"][2] == 0 and skipped["iters_run"][1] > 0
    e = ac.empty_source_case(None).want()
    assert e["status"] == 2 and e["iters_run"] == [0, 0, 1] and e["pairs"] == 0
