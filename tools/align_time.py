"""Times registering one volume against another (tsdf_align_volume, tsdf_align_system, csrc/tsdf_align.hip.h) on the GPU.

    python tools/align_time.py [--repeats 50] [--warmup 3] [--edge 200] [--step-seconds 60] [--out FILE]

Two volumes of edge^3 @ 4 mm hold one scene without symmetry (synth.TrackScene), the source fused from 16 views, the
destination from 8 others; the destination's base2world is off by 2 degrees about the grid's centre and 3 mm.  Steps, in one
run on one pair of handles: tsdf_align_volume at the default schedule; one tsdf_align_system pass at level 0 and at level 1
at the starting pose; and tsdf_fuse_volume with write = 0, the sibling that makes the same 16 gathers for EVERY destination
voxel inside the source's box where align_pairs makes them for the candidates only.  Every figure is the host clock around one
synchronous call (each ends with its own stream synchronise; the align calls include the state's initialisation and copy
back).  Beside the times: the lattice sizes, the pairs and iterations of the run, and the merge's counts at the start and at
the result.  A step stops early, and says so, when it has used --step-seconds.
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from semantic_slam_amd import capi, synth  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--repeats", type=int, default=50)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--edge", type=int, default=200)
ap.add_argument("--step-seconds", type=float, default=60.0)
ap.add_argument("--out", default="")
args = ap.parse_args()
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def spread(ms):
    ms = np.sort(np.asarray(ms))
    return (f"median {np.median(ms):.4f} ms, min {ms[0]:.4f}, p10 {np.percentile(ms, 10):.4f}, p90 {np.percentile(ms, 90):.4f}, "
            f"max {ms[-1]:.4f} (n = {len(ms)})")


def timed(call):
    """Median-ready list of milliseconds of `call`; stops at the step's time limit."""
    t_end = time.perf_counter() + args.step_seconds
    ms = []
    for i in range(args.warmup + args.repeats):
        t0 = time.perf_counter()
        call()
        dt = (time.perf_counter() - t0) * 1e3
        if i >= args.warmup:
            ms.append(dt)
        if time.perf_counter() > t_end and ms:
            say(f"    (step stopped at its time limit after {len(ms)} timed calls)")
            break
    return ms


E, vs = args.edge, 0.004
dims = (E, E, E)
origin = synth.surf_volume(E, vs, 0.8)
centre = origin.astype(np.float64) + E * vs / 2
R = synth.rot_y(np.radians(2.0))
T = np.eye(4)
T[:3, :3] = R
T[:3, 3] = centre - R @ centre + np.array([0.003, -0.003, 0.003])
scene = synth.TrackScene(dims, vs, origin)
poses = [scene.pose(k, n=24) for k in range(24)]
depths = [torch.from_numpy(scene.depth(c, quantize=True)).cuda() for c in poses]
src_cfg = capi.make_config(dims, vs, origin)
true_cfg = capi.make_config(dims, vs, origin)
dst_cfg = capi.make_config(dims, vs, origin, base2world=T.astype(np.float32).ravel())      # what the handle believes
say(f"source and destination {E}^3 @ 4 mm ({2 * 4 * E ** 3 / 1e6:.0f} MB each), one scene; source 16 frames, destination 8; "
    f"the destination's base2world off by 2 deg + 3 mm")
with capi.Volume(src_cfg) as src, capi.Volume(true_cfg) as fused, capi.Volume(dst_cfg) as dst:
    src.integrate_frames_device([d.data_ptr() for d in depths[:16]], np.stack(poses[:16]))
    fused.integrate_frames_device([d.data_ptr() for d in depths[16:]], np.stack(poses[16:]))
    dst.upload(*fused.download())                             # the content of the true pose under the wrong base2world
    src.sync()
    t, w = dst.download()
    p = capi.align_params_default(dst_cfg)
    start = capi.fuse_pose_default(dst_cfg, src_cfg)
    dry = capi.fuse_params_default(dst_cfg)
    dry.write = 0
    say(f"  lattice: level 0 {E ** 3} points, level 1 {((E + 1) // 2) ** 3}; candidates at level 0 (weight > {p.weight_thresh:.1f}, "
        f"|tsdf| < 1): {int(((w > p.weight_thresh) & (np.abs(t) < 1)).sum())}")
    out = {}
    ms_fuse = timed(lambda: out.update(dst.fuse_from(src, dry)))
    say(f"  tsdf_fuse_volume, write = 0, at the starting pose: {spread(ms_fuse)}; counts {out}")
    for level in (0, 1):
        ms = timed(lambda: out.update(n=dst.align_system(src, start, level=level, params=p)[3]))
        say(f"  tsdf_align_system, level {level}: {spread(ms)}; {np.median(ms) / np.median(ms_fuse):.2f} x the dry merge; pairs {out['n']}")
    ms = timed(lambda: out.update(r=dst.align_to(src, params=p)))
    pose, st = out["r"]
    say(f"  tsdf_align_volume, default schedule {list(p.iters)[:p.n_levels]}: {spread(ms)}; {np.median(ms) / np.median(ms_fuse):.2f} x the "
        f"dry merge; {sum(st['iters_run'])} iterations {st['iters_run']}, {np.median(ms) / max(1, sum(st['iters_run'])):.4f} ms each; "
        f"status {st['status_name']}, pairs {st['pairs']}, rmse {st['rmse']:.4f}")
    after = dst.fuse_from(src, dry, dst2src=pose)
    ratio = lambda c: c["agree_band"] / max(1, c["both_band"])
    say(f"  agree_band / both_band: {ratio(dst.fuse_from(src, dry)):.4f} at the starting pose, {ratio(after):.4f} at the result")

if args.out:
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
