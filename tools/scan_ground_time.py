"""Times marking a scan's ground (tsdf_scan_mark_ground, tsdf_scan_project_ground, tsdf_integrate_scan_ground;
csrc/tsdf_scan_ground.hip.h) on the GPU, beside the calls it sits in front of.

    python tools/scan_ground_time.py [--repeats 60] [--warmup 5] [--out profiles/rNN_scan_ground_time.txt]

The scan, calibration and volume of tools/scan_time.py: one synthetic 64-beam scan (~119 000 points) through the KITTI
2011_09_30 calibration of tests/golden into a 1242 x 375 image; a 200^3 @ 2 cm volume around the cube, deferral off so that
every call launches; the ground parameters that fit the sensor (64 x 4500 cells, each beam at its ring's centre, the upper
cell marked), TSDF_SCAN_DROP_GROUND, the fill's default parameters.  Timed in turn, one call of each per round, so that all
of them see the same box at the same time; every other round runs the calls in the reverse order, so that no call always
follows the same neighbour:

  tsdf_scan_mark_ground                          points in; flags, states, winners and counts out, on the host
  tsdf_scan_project_ground                       points in, filled depth image of the kept points, kinds and counts out
  tsdf_integrate_scan + sync                     points in, fused: every point, unfilled
  tsdf_integrate_scan_ground + sync              ... without the ground returns
  tsdf_integrate_scan_filled + sync              points in, fused: every point, filled
  tsdf_integrate_scan_ground (filled) + sync     ... without the ground returns
  NumPy restatement                              tests/scan_ground_spec.py on this box's CPU, the marking alone, vectorised;
                                                 timed after the rounds, so that the device does not idle between the others

Every timed window ends with the work finished (the scanner calls return with their outputs, the others are followed by
tsdf_sync), so a host clock around it is a timing of finished work.  These are recorded figures, not thresholds.
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import scan_cases  # noqa: E402
import scan_ground_cases as cases  # noqa: E402
import scan_ground_spec as spec  # noqa: E402
from semantic_slam_amd import capi  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--repeats", type=int, default=60)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--numpy-calls", type=int, default=3)
ap.add_argument("--out", default="")
args = ap.parse_args()
assert args.repeats >= 50, "the record wants at least 50 calls"
assert torch.cuda.is_available(), "this tool measures on the GPU"
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def spread(ms):
    ms = np.sort(np.asarray(ms))
    return f"p10 {np.percentile(ms, 10):.4f} ms, median {np.median(ms):.4f}, p90 {np.percentile(ms, 90):.4f} (n = {len(ms)})"


s = scan_cases.calibration_case()
c = cases.kitti_marks("hdl64e_upper")
pts, velo2img, K, H, W = s["points"], s["velo2img"], s["K"], s["H"], s["W"]
scene = scan_cases.kitti_scene()
pose = scene.pose(0, n=16, max_yaw_deg=5.0)
cfg = capi.make_config(scene.dims, scene.vs, scene.origin.astype(np.float32), K=K, im_height=H, im_width=W, max_depth=80.0)
ground = spec.to_capi(c["params"])
fill = capi.scan_fill_params_default()
DROP = capi.SCAN_DROP_GROUND

with capi.Volume(cfg) as v_scan, capi.Volume(cfg) as v_ground, capi.Volume(cfg) as v_filled, capi.Volume(cfg) as v_ground_filled, \
        capi.Scanner(H, W) as sc:
    for v in (v_scan, v_ground, v_filled, v_ground_filled):
        v.set_deferral(0)

    def synced(vol, fn):
        def call():
            fn()
            vol.sync()
        return call

    calls = {
        "tsdf_scan_mark_ground": lambda: sc.mark_ground(pts, ground),
        "tsdf_scan_project_ground": lambda: sc.project_ground(pts, velo2img, K, ground, DROP, fill_params=fill, want_range=False),
        "tsdf_integrate_scan + sync": synced(v_scan, lambda: v_scan.integrate_scan(pts, velo2img, pose)),
        "tsdf_integrate_scan_ground + sync": synced(v_ground, lambda: v_ground.integrate_scan_ground(pts, velo2img, pose, ground, DROP)),
        "tsdf_integrate_scan_filled + sync": synced(v_filled, lambda: v_filled.integrate_scan_filled(pts, velo2img, pose, fill)),
        "tsdf_integrate_scan_ground (filled) + sync": synced(v_ground_filled, lambda: v_ground_filled.integrate_scan_ground(
            pts, velo2img, pose, ground, DROP, fill_params=fill)),
    }
    ms = {k: [] for k in calls}
    last = {}
    for i in range(args.warmup + args.repeats):
        for name, fn in (list(calls.items())[::-1] if i % 2 else calls.items()):
            t0 = time.perf_counter()
            last[name] = fn()
            dt = (time.perf_counter() - t0) * 1e3
            if i >= args.warmup:
                ms[name].append(dt)
    w = c["want"]
    say(f"{len(pts)} points into {c['params'].n_rings} x {c['params'].n_columns} cells ({w['counts'][1]} occupied, {w['counts'][2]} ground; "
        f"{w['counts'][3]} ground points) and {W} x {H}, {scene.dims[0]}^3 @ {scene.vs * 100:.0f} cm volume, deferral off, host clock per "
        f"call, one call of each per round, the order reversed every other round:")
    for name in calls:
        say(f"  {name:44s} {spread(ms[name])}")
    numpy_ms = []
    for _ in range(args.numpy_calls):
        t0 = time.perf_counter()
        spec.mark(pts, c["params"], c["tab"])
        numpy_ms.append((time.perf_counter() - t0) * 1e3)
    say(f"  {'NumPy restatement':44s} {spread(numpy_ms)}")
    flags, state, winner, counts = last["tsdf_scan_mark_ground"]
    assert flags.tobytes() == w["flags"].tobytes() and state.tobytes() == w["state"].tobytes() and winner.tobytes() == w["winner"].tobytes()
    assert list(counts) == list(w["counts"])
    assert last["tsdf_scan_project_ground"]["n_selected"] == len(pts) - w["counts"][3]
    say("  the device's flags, states, winners and counts equal the restatement's")
    for name, vol in (("every point", v_scan), ("without the ground", v_ground), ("every point, filled", v_filled),
                      ("without the ground, filled", v_ground_filled)):
        say(f"  voxels updated per frame, {name}: {np.count_nonzero(vol.download()[1])}")

if args.out:
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
