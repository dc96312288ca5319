"""Times the merge that carries colour and labels (tsdf_fuse_volume_carry, csrc/tsdf_fuse_carry.hip.h) on the GPU, beside
the geometry-only merge of the same pair.

    python tools/fuse_carry_time.py [--repeats 50] [--warmup 3] [--edge 200] [--out FILE]

Two volumes of edge^3 @ 4 mm hold the same scene (synth.SurfScene) with colour and labels, the source fused from 16 views, the
destination from 8 others whose label images put the instance boundary elsewhere.  For a small rotation (2 degrees about the
grid's centre, 3 mm shift) and for the aligned case, with write = 1, five calls are timed in turn within every round, so
that drift of the machine meets all of them alike: tsdf_fuse_volume_at (the yardstick: its kernel is the geometry-only one)
and tsdf_fuse_volume_carry with carry = 0, 1 (colour), 2 (labels) and 3, all at the same pose.  Every figure is the host clock
around one synchronous call.  Before every call the destination's six arrays are restored by the uploads, outside the clock,
so each call merges into the same state.
"""
import argparse
import ctypes as C
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
ap.add_argument("--out", default="")
args = ap.parse_args()
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def spread(ms):
    return f"median {np.median(ms):.4f} ms (p10 {np.percentile(ms, 10):.4f} - p90 {np.percentile(ms, 90):.4f}, n = {len(ms)})"


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
h, w = synth.IM_H, synth.IM_W
v, u = np.mgrid[0:h, 0:w]
rgbs = [torch.from_numpy(np.stack([(u + 9 * k) % 256, (2 * v + 5 * k) % 256, (u + v) % 256], -1).astype(np.uint8)).cuda()
        for k in range(24)]
score = torch.from_numpy(np.full((h, w), 0.8, np.float32)).cuda()
label_ims = {side: torch.from_numpy(np.where(u < at, 1, 2).astype(np.uint16)).cuda() for side, at in (("src", w // 2), ("dst", 2 * w // 5))}
src_cfg = capi.make_config(dims, vs, origin)
lib = capi.load()


def feed(vol, side, frames):
    vol.colour_enable()
    vol.labels_enable(0.5)
    for k in frames:
        vol.integrate_device(depths[k].data_ptr(), poses[k])
        vol.integrate_colour_device(depths[k].data_ptr(), rgbs[k].data_ptr(), poses[k])
        vol.integrate_labels_device(depths[k].data_ptr(), label_ims[side].data_ptr(), score.data_ptr(), poses[k])
    vol.sync()


say(f"source and destination {E}^3 @ 4 mm, one scene with colour and labels; source 16 frames, destination 8; write = 1")
for name, b2w in (("rotated 2 deg + 3 mm", T.astype(np.float32).ravel()), ("aligned", np.eye(4, dtype=np.float32).ravel())):
    dst_cfg = capi.make_config(dims, vs, origin, base2world=b2w)
    with capi.Volume(src_cfg) as src, capi.Volume(dst_cfg) as dst:
        feed(src, "src", range(16))
        feed(dst, "dst", range(16, 24))
        t0, w0 = dst.download()
        c0, (l0, f0, b0) = dst.download_colour(), dst.download_labels()
        pose = capi.fuse_pose_default(dst_cfg, src_cfg)
        p = capi.fuse_params_default(dst_cfg)
        counts, carried = capi.FuseCounts(), capi.FuseCarryCounts()

        def restore():
            dst.upload(t0, w0)
            dst.upload_colour(c0)
            dst.upload_labels(l0, f0, b0)

        def merge_at():
            capi.check(lib.tsdf_fuse_volume_at(dst._h, src._h, C.byref(p), pose.ctypes.data, C.byref(counts)), "tsdf_fuse_volume_at")

        def merge_carry(carry):
            capi.check(lib.tsdf_fuse_volume_carry(dst._h, src._h, C.byref(p), pose.ctypes.data, carry, C.byref(counts),
                                                  C.byref(carried)), "tsdf_fuse_volume_carry")

        calls = [("tsdf_fuse_volume_at", merge_at)] + [(f"tsdf_fuse_volume_carry, carry = {c}", lambda c=c: merge_carry(c))
                                                       for c in (0, 1, 2, 3)]
        ms = {label: [] for label, _ in calls}
        for i in range(args.warmup + args.repeats):
            for label, call in calls:
                restore()
                t_start = time.perf_counter()
                call()
                dt = (time.perf_counter() - t_start) * 1e3
                if i >= args.warmup:
                    ms[label].append(dt)
        say(f"  {name}: sampled {counts.sampled}; labels adopted {carried.label_adopted}, agreed {carried.label_agreed}, "
            f"opposed {carried.label_opposed}, flipped {carried.label_flipped}")
        base = ms["tsdf_fuse_volume_at"]
        lo, hi = np.percentile(base, 10), np.percentile(base, 90)
        for label, _ in calls:
            note = f"; {np.median(ms[label]) / np.median(base):.2f} x tsdf_fuse_volume_at"
            if label.endswith("= 0"):
                inside = lo <= np.median(ms[label]) <= hi
                note += f"; median {'inside' if inside else 'OUTSIDE'} that call's p10 - p90"
            say(f"    {label}: {spread(ms[label])}{'' if label == 'tsdf_fuse_volume_at' else note}")

if args.out:
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
