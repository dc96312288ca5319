"""Times the lidar path (tsdf_scan_project, tsdf_integrate_scan; csrc/tsdf_scan.hip.h) on the GPU.

    python tools/scan_time.py [--repeats 60] [--warmup 5] [--out profiles/r19_scan_time.txt]

One synthetic 64-beam scan (~119 000 points, every ray returns) of a 4 m S-surf cube six metres ahead, through the KITTI
2011_09_30 calibration of tests/golden into a 1242 x 375 image; a 200^3 @ 2 cm volume around the cube, deferral off so that
every call launches.  Timed in turn, one call of each per round, so that all of them see the same box at the same time:

  tsdf_scan_project              points in, range and depth images and the pixel count out, on the host when it returns
  tsdf_integrate_scan + sync     points in, fused: copy, splat, resolve into the frame's slot, Integrate
  tsdf_integrate + sync          the ready depth image of the same scan on the same handle: what the call above adds to
  NumPy restatement              tests/scan_spec.py on this box's CPU: projection and conversion, vectorised

Every timed window ends with the work finished (the first call returns with its images, the others are followed by
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
import scan_cases as cases  # noqa: E402
import scan_spec as spec  # noqa: E402
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


c = cases.calibration_case()
pts, velo2img, K, H, W = c["points"], c["velo2img"], c["K"], c["H"], c["W"]
scene = cases.kitti_scene()
pose = scene.pose(0, n=16, max_yaw_deg=5.0)
cfg = capi.make_config(scene.dims, scene.vs, scene.origin.astype(np.float32), K=K, im_height=H, im_width=W, max_depth=80.0)
depth = c["depth"]

with capi.Volume(cfg) as vol, capi.Scanner(H, W) as sc:
    vol.set_deferral(0)

    def integrate_scan():
        vol.integrate_scan(pts, velo2img, pose)
        vol.sync()

    def integrate_depth():
        vol.integrate(depth, pose)
        vol.sync()

    calls = {
        "tsdf_scan_project": lambda: sc.project(pts, velo2img, K),
        "tsdf_integrate_scan + sync": integrate_scan,
        "tsdf_integrate + sync": integrate_depth,
        "NumPy restatement": lambda: spec.scan_depth(pts, velo2img, K, H, W),
    }
    ms = {k: [] for k in calls}
    last = {}
    for i in range(args.warmup + args.repeats):
        for name, fn in calls.items():
            t0 = time.perf_counter()
            last[name] = fn()
            dt = (time.perf_counter() - t0) * 1e3
            if i >= args.warmup:
                ms[name].append(dt)
    say(f"{len(pts)} points into {W} x {H} ({c['n_pixels']} written pixels), {scene.dims[0]}^3 @ {scene.vs * 100:.0f} cm volume, "
        f"deferral off, host clock per call, one call of each per round:")
    for name in calls:
        say(f"  {name:30s} {spread(ms[name])}")
    rng, dep, n = last["tsdf_scan_project"]
    assert n == c["n_pixels"] and rng.tobytes() == c["range"].tobytes() and dep.tobytes() == depth.tobytes()
    assert last["NumPy restatement"].tobytes() == depth.tobytes()
    say("  the device's images equal the restatement's bit for bit")

if args.out:
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
