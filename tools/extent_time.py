"""Times the extent reduction (tsdf_volume_extent, tsdf_batch_extents, csrc/tsdf_extent.hip.h) on the GPU.

    python tools/extent_time.py [--repeats 50] [--warmup 5] [--members 16] [--edge 200] [--big 512] [--step-seconds 60] [--out FILE]

Three steps in one run: tsdf_batch_extents over `members` volumes of edge^3 @ 4 mm, each fused from 8 views of one scene
(synth.SurfScene); tsdf_volume_extent on one big^3 handle fused from 8 views; and, on the same handle, tsdf_count_surface,
which reads the same two arrays and serves as the yardstick.  Every figure is the host clock around one synchronous call
(each ends with its own stream synchronise and includes the finishing launch and the record's copy).  The reduction reads
8 bytes per voxel; the rate is those bytes over the median, as a fraction of the 8 TB/s peak of the MI355X's HBM.  A step
stops early, and says so, when it has used --step-seconds.
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
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--members", type=int, default=16)
ap.add_argument("--edge", type=int, default=200)
ap.add_argument("--big", type=int, default=512)
ap.add_argument("--step-seconds", type=float, default=60.0)
ap.add_argument("--out", default="")
args = ap.parse_args()
lines = []
PEAK_TBS = 8.0


def say(s):
    print(s, flush=True)
    lines.append(s)


def spread(ms):
    ms = np.sort(np.asarray(ms))
    return (f"median {np.median(ms):.4f} ms, min {ms[0]:.4f}, p10 {np.percentile(ms, 10):.4f}, p90 {np.percentile(ms, 90):.4f}, "
            f"max {ms[-1]:.4f} (n = {len(ms)})")


def rate(voxels, ms):
    tbs = 8.0 * voxels / (np.median(ms) * 1e-3) / 1e12
    return f"{tbs:.2f} TB/s on 8 B per voxel, {100 * tbs / PEAK_TBS:.0f} % of the {PEAK_TBS:.0f} TB/s peak"


def timed(call):
    """List of milliseconds of `call` after the warm-up calls; stops at the step's time limit."""
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


def fused_frames(edge, vs=0.004, n=8):
    origin = synth.surf_volume(edge, vs, 0.8)
    scene = synth.SurfScene((edge,) * 3, vs, origin)
    poses = [scene.pose(k, n=24) for k in range(n)]
    return origin, np.stack(poses), [torch.from_numpy(scene.depth(c, quantize=True)).cuda() for c in poses]


vs = 0.004
E, M = args.edge, args.members
origin, poses, depths = fused_frames(E)
cfgs = [capi.make_config((E, E, E), vs, origin, vol_id=i) for i in range(M)]
p = capi.extent_params_default(cfgs[0])
say(f"parameters: weight_thresh {p.weight_thresh:.1f}, band {p.band:.1f}, margin {p.margin}")
with capi.Batch(cfgs) as batch:
    for c2w, d in zip(poses, depths):
        batch.integrate_device(d.data_ptr(), None, c2w)
    batch.sync()
    recs = batch.extents(p)
    ms = timed(lambda: batch.extents(p))
    e = recs[0]
    say(f"tsdf_batch_extents, {M} members of {E}^3 ({8 * M * E ** 3 / 1e6:.0f} MB read), one launch: {spread(ms)}; "
        f"{rate(M * E ** 3, ms)}")
    say(f"    member 0: observed {e.n_observed}, surface {e.n_surface}, lo {list(e.lo)}, hi {list(e.hi)}, border {list(e.border)}")
    one = timed(lambda: batch.volumes[0].extent(p))
    say(f"tsdf_volume_extent on one of those members ({8 * E ** 3 / 1e6:.0f} MB read): {spread(one)}; {rate(E ** 3, one)}")
del depths

B = args.big
origin, poses, depths = fused_frames(B)
cfg = capi.make_config((B, B, B), vs, origin)
with capi.Volume(cfg) as vol:
    vol.integrate_frames_device([d.data_ptr() for d in depths], poses)
    vol.sync()
    e = vol.extent(p)
    n_count = vol.count_surface(p.weight_thresh)
    # the two calls alternate, so that neither has the quieter half of the run
    t_end = time.perf_counter() + 2 * args.step_seconds
    ms_e, ms_c = [], []
    for i in range(args.warmup + args.repeats):
        t0 = time.perf_counter()
        vol.extent(p)
        t1 = time.perf_counter()
        vol.count_surface(p.weight_thresh)
        t2 = time.perf_counter()
        if i >= args.warmup:
            ms_e.append((t1 - t0) * 1e3)
            ms_c.append((t2 - t1) * 1e3)
        if time.perf_counter() > t_end and ms_e:
            say(f"    (step stopped at its time limit after {len(ms_e)} timed calls)")
            break
    say(f"tsdf_volume_extent, one {B}^3 handle ({8 * B ** 3 / 1e6:.0f} MB read): {spread(ms_e)}; {rate(B ** 3, ms_e)}")
    say(f"    observed {e.n_observed}, surface {e.n_surface}, lo {list(e.lo)}, hi {list(e.hi)}, border {list(e.border)}")
    say(f"tsdf_count_surface on the same handle, alternating with it: {spread(ms_c)}; {rate(B ** 3, ms_c)}; count {n_count}")
    say(f"ratio tsdf_volume_extent / tsdf_count_surface (medians): {np.median(ms_e) / np.median(ms_c):.2f}")

if args.out:
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
