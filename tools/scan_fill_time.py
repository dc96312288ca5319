"""Times the lidar gap fill (tsdf_scan_fill_depth, tsdf_scan_project_filled, tsdf_integrate_scan_filled;
csrc/tsdf_scan_fill.hip.h) on the GPU, beside the unfilled calls it sits behind.

    python tools/scan_fill_time.py [--repeats 60] [--warmup 5] [--out profiles/r20_scan_fill_time.txt]

The scan, calibration and volume of tools/scan_time.py: one synthetic 64-beam scan (~119 000 points) through the KITTI
2011_09_30 calibration of tests/golden into a 1242 x 375 image; a 200^3 @ 2 cm volume around the cube, deferral off so that
every call launches; the fill's default parameters.  Timed in turn, one call of each per round, so that all of them see the
same box at the same time; every other round runs the calls in the reverse order, so that no call always follows the same
neighbour:

  tsdf_scan_fill_depth               a sparse depth image in, the filled image, the kinds and the count out, on the host
  tsdf_scan_project                  points in, depth image out (no range image, no count): what the next call adds to
  tsdf_scan_project_filled           points in, filled depth image, kinds and count out
  tsdf_integrate_scan + sync         points in, fused unfilled
  tsdf_integrate_scan_filled + sync  points in, fused filled: thirteen times as many voxels pass Integrate's tests
  NumPy restatement                  tests/scan_fill_spec.py on this box's CPU, the fill alone, vectorised; timed after the
                                     rounds, ten calls, so that its 25 ms of an idle device do not sit between the others

Every timed window ends with the work finished (the scanner calls return with their images, the others are followed by
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
import scan_fill_cases as cases  # noqa: E402
import scan_fill_spec as spec  # noqa: E402
from semantic_slam_amd import capi  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--repeats", type=int, default=60)
ap.add_argument("--warmup", type=int, default=5)
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
c = cases.kitti_case()
pts, velo2img, K, H, W = s["points"], s["velo2img"], s["K"], s["H"], s["W"]
scene = scan_cases.kitti_scene()
pose = scene.pose(0, n=16, max_yaw_deg=5.0)
cfg = capi.make_config(scene.dims, scene.vs, scene.origin.astype(np.float32), K=K, im_height=H, im_width=W, max_depth=80.0)
params = capi.scan_fill_params_default()

with capi.Volume(cfg) as vol, capi.Volume(cfg) as vol_filled, capi.Scanner(H, W) as sc:
    vol.set_deferral(0)
    vol_filled.set_deferral(0)

    def integrate_scan():
        vol.integrate_scan(pts, velo2img, pose)
        vol.sync()

    def integrate_scan_filled():
        vol_filled.integrate_scan_filled(pts, velo2img, pose, params)
        vol_filled.sync()

    calls = {
        "tsdf_scan_fill_depth": lambda: sc.fill_depth(c["depth"], params),
        "tsdf_scan_project": lambda: sc.project(pts, velo2img, K, want_range=False, want_count=False),
        "tsdf_scan_project_filled": lambda: sc.project_filled(pts, velo2img, K, params),
        "tsdf_integrate_scan + sync": integrate_scan,
        "tsdf_integrate_scan_filled + sync": integrate_scan_filled,
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
    say(f"{len(pts)} points into {W} x {H} ({s['n_pixels']} measured pixels, {c['n_filled']} filled with spans {c['params'][0]}, "
        f"{c['params'][1]} and jump {c['params'][2]:.2f}), {scene.dims[0]}^3 @ {scene.vs * 100:.0f} cm volume, deferral off, "
        f"host clock per call, one call of each per round, the order reversed every other round:")
    for name in calls:
        say(f"  {name:36s} {spread(ms[name])}")
    numpy_ms = []
    for _ in range(10):
        t0 = time.perf_counter()
        spec.fill(c["depth"], *c["params"])
        numpy_ms.append((time.perf_counter() - t0) * 1e3)
    say(f"  {'NumPy restatement':36s} {spread(numpy_ms)}")
    for name in ("tsdf_scan_fill_depth", "tsdf_scan_project_filled"):
        f, k, n = last[name]
        assert n == c["n_filled"] and f.tobytes() == c["filled"].tobytes() and k.tobytes() == c["kind"].tobytes(), name
    assert last["tsdf_scan_project"][1].tobytes() == c["depth"].tobytes()
    say("  the device's images equal the restatement's bit for bit")
    _, w_s = vol.download()
    _, w_f = vol_filled.download()
    say(f"  voxels updated per frame: {np.count_nonzero(w_s)} unfilled, {np.count_nonzero(w_f)} filled")

if args.out:
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
