"""Times merging one volume into another (tsdf_fuse_volume, csrc/tsdf_fuse.hip.h) on the GPU.

    python tools/fuse_time.py [--repeats 50] [--warmup 3] [--edge 200] [--step-seconds 60] [--out FILE]

Two volumes of edge^3 @ 4 mm hold the same scene (synth.SurfScene), the source fused from 16 views, the destination from 8
others.  Steps: a merge under a small rotation (2 degrees about the grid's centre, 3 mm shift) with write = 0 and write = 1;
the same for the aligned case (both grids in one place); and, on the same stream in the same run, a device-to-device copy
of the destination's two arrays (tsdf_copy_slices into device buffers) -- the floor for a kernel that must read and write
the destination.  Every figure is the host clock around one synchronous call (tsdf_fuse_volume ends with its own stream
synchronise and includes the counts' zeroing and copy, and for write = 1 the rebuild of the free-space summary).  Before
every writing call the destination is restored by tsdf_upload, outside the clock, so each call merges into the same state.
A step stops early, and says so, when it has used --step-seconds.
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


def timed(call, before=None):
    """Median-ready list of milliseconds of `call`, `before` run outside the clock; stops at the step's time limit."""
    t_end = time.perf_counter() + args.step_seconds
    ms = []
    for i in range(args.warmup + args.repeats):
        if before:
            before()
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
scene = synth.SurfScene(dims, vs, origin)
poses = [scene.pose(k, n=24) for k in range(24)]
depths = [torch.from_numpy(scene.depth(c, quantize=True)).cuda() for c in poses]
src_cfg = capi.make_config(dims, vs, origin)
say(f"source and destination {E}^3 @ 4 mm ({2 * 4 * E ** 3 / 1e6:.0f} MB each), one scene; source 16 frames, destination 8")
copy_ms = None
for name, b2w in (("rotated 2 deg + 3 mm", T.astype(np.float32).ravel()), ("aligned", np.eye(4, dtype=np.float32).ravel())):
    dst_cfg = capi.make_config(dims, vs, origin, base2world=b2w)
    with capi.Volume(src_cfg) as src, capi.Volume(dst_cfg) as dst:
        src.integrate_frames_device([d.data_ptr() for d in depths[:16]], np.stack(poses[:16]))
        dst.integrate_frames_device([d.data_ptr() for d in depths[16:]], np.stack(poses[16:]))
        src.sync()
        t0, w0 = dst.download()
        if copy_ms is None:
            ct = torch.empty(E ** 3, dtype=torch.float32, device="cuda")
            cw = torch.empty(E ** 3, dtype=torch.float32, device="cuda")
            copy_ms = timed(lambda: dst.copy_slices_to_device(0, E, ct.data_ptr(), cw.data_ptr()))
            say(f"  device-to-device copy of the destination's two arrays (reads and writes {4 * 4 * E ** 3 / 1e6:.0f} MB): "
                f"{spread(copy_ms)}")
            del ct, cw
        for write in (0, 1):
            p = capi.fuse_params_default(dst_cfg)
            p.write = write
            out = {}
            ms = timed(lambda: out.update(dst.fuse_from(src, p)), before=(lambda: dst.upload(t0, w0)) if write else None)
            say(f"  {name}, write = {write}: {spread(ms)}; {np.median(ms) / np.median(copy_ms):.2f} x the copy; counts {out}")

if args.out:
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
