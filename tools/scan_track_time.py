"""Times scan tracking (tsdf_scan_track, tsdf_scan_track_system; csrc/tsdf_scan_track.hip.h) on the GPU.

    python tools/scan_track_time.py [--repeats 60] [--warmup 5] [--out profiles/r22_scan_track_time.txt]

The synthetic 64-beam scan of tools/scan_time.py (~119 000 points, every ray returns, firing order) of a 4 m S-surf cube six
metres ahead, through the KITTI 2011_09_30 calibration of tests/golden; the model is a 512^3 volume over the cube (2^-7 m
voxels, truncation 39 mm) fused from the gap-filled camera views of eight such scans along the scene's orbit
(tsdf_integrate_scan_filled), the tracked scan a ninth from a pose between them, its guess 0.5 degrees and 15 mm off.  Default
parameters.  Timed in turn, one call of each per round, so that all of them see the same box at the same time:

  tsdf_scan_track_system, level l   one pass over every 2^l-th point and the summed system, on the host when it returns
  tsdf_scan_track                   the whole track: upload, every iteration of every level, the result on the host
  tsdf_track                        the camera tracker on the same scan's gap-filled 1242 x 375 depth image (in HBM
                                    already), from the same guess: the render, its iterations, the result on the host

Every call returns with its result on the host, so a host clock around it is a timing of finished work.  These are recorded
figures, not thresholds: nobody has measured this before.
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
import scan_track_cases as stc  # noqa: E402
import scan_track_spec as sts  # noqa: E402
from semantic_slam_amd import capi, synth  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--repeats", type=int, default=60)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--dim", type=int, default=512)
ap.add_argument("--out", default="")
args = ap.parse_args()
assert torch.cuda.is_available(), "this tool measures on the GPU"
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def spread(ms):
    ms = np.sort(np.asarray(ms))
    return f"p10 {np.percentile(ms, 10):.4f} ms, median {np.median(ms):.4f}, p90 {np.percentile(ms, 90):.4f} (n = {len(ms)})"


cal = cases.golden_calibration()
c = cases.calibration_case()
velo2img, K, H, W = c["velo2img"], c["K"], c["H"], c["W"]
E = args.dim
vs = 4.0 / E
scene = synth.SurfScene((E,) * 3, vs, np.array([-2.0, -2.0, 4.0]), h=H, w=W)
cfg = capi.make_config(scene.dims, vs, scene.origin.astype(np.float32), K=K, im_height=H, im_width=W, max_depth=80.0)
# the camera velo2img projects into: tsdf_scan_pose's rectified camera moved by P_rect's fourth column (camera 2's baseline)
velo2cam = np.eye(4)
velo2cam[:3] = np.linalg.inv(np.asarray(K, np.float64).reshape(3, 3)) @ np.asarray(velo2img, np.float64).reshape(3, 4)
assert np.allclose(velo2cam[:3, :3], capi.scan_pose(cal["R_rect"], cal["R_velo"], cal["t_velo"])[:3, :3], atol=1e-5)
velo2cam = velo2cam.astype(np.float32).ravel()
room = (40.0, 25.0, 10.0, 1.73)


def scan_at(pose):
    """The scan of a sensor mounted at velo2cam on the camera at `pose`: the mount the fused images are made with, so that the
    model and the scan are one scene."""
    return synth.lidar_scan(scene, pose, velo2cam.reshape(4, 4), room=room)


with capi.Volume(cfg) as vol, capi.Scanner(H, W) as scanner:
    for k in range(0, 16, 2):
        pose = scene.pose(k, n=16, max_yaw_deg=5.0)
        vol.integrate_scan_filled(scan_at(pose), velo2img, pose)
    vol.sync()
    cam_true = scene.pose(3, n=16, max_yaw_deg=5.0)
    pts = scan_at(cam_true)
    truth = capi.multiply_matrix(cam_true, velo2cam)
    guess = stc.moved(truth, 0.5, 0.015, 3)
    _, cam2velo = capi.invert_matrix(velo2cam)
    cam_guess = capi.multiply_matrix(guess, cam2velo)
    p = capi.scan_track_params_default(cfg)
    depth, _, n_filled = scanner.project_filled(pts, velo2img, K, want_kind=False)
    depth_dev = torch.from_numpy(depth).cuda()
    tp = capi.track_params_default(cfg)

    calls = {f"tsdf_scan_track_system, level {l}": (lambda l=l: vol.track_scan_system(pts, guess, level=l, params=p)) for l in range(3)}
    calls["tsdf_scan_track"] = lambda: vol.track_scan(pts, guess, params=p)
    calls["tsdf_track (filled depth image)"] = lambda: vol.track(depth_dev.data_ptr(), cam_guess, params=tp)
    ms = {k: [] for k in calls}
    last = {}
    for i in range(args.warmup + args.repeats):
        for name, fn in calls.items():
            t0 = time.perf_counter()
            last[name] = fn()
            dt = (time.perf_counter() - t0) * 1e3
            if i >= args.warmup:
                ms[name].append(dt)
    say(f"{len(pts)} points against a {E}^3 @ {vs * 1e3:.2f} mm volume fused from 8 gap-filled scans, default parameters, host clock "
        f"per call, one call of each per round:")
    for name in calls:
        say(f"  {name:34s} {spread(ms[name])}")
    for l in range(3):
        say(f"  level {l}: {int(last[f'tsdf_scan_track_system, level {l}'][28])} pairs of {-(-len(pts) // (1 << l))} points")
    got, st = last["tsdf_scan_track"]
    (r0, t0), (r1, t1) = sts.pose_error(guess, truth), sts.pose_error(got, truth)
    say(f"  tsdf_scan_track: {st}; {r0:.3f} deg {1e3 * t0:.1f} mm -> {r1:.3f} deg {1e3 * t1:.1f} mm from the pose the scan was cast at")
    got_c, st_c = last["tsdf_track (filled depth image)"]
    r2, t2 = sts.pose_error(capi.multiply_matrix(got_c.ravel(), velo2cam), truth)
    say(f"  tsdf_track: {st_c}; -> {r2:.3f} deg {1e3 * t2:.1f} mm ({int(np.count_nonzero(depth))} depth pixels, {n_filled} of them filled)")

if args.out:
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
