"""Times geometric segmentation and mask refinement (tsdf_segment_*, csrc/tsdf_segment.hip.h) on the GPU.

    python tools/segment_time.py [--repeats 50] [--warmup 5] [--ks 4,16,64] [--spec] [--out FILE]

The frame: synth.ObjectScene() at pose 3, 640 x 480, default parameters.  The K instance masks are the four objects' masks
dilated by 6 pixels, repeated to K.  Per call the host clock runs around it; every call ends with its own stream synchronise,
so the time covers the launches, the kernels, the copy of the cluster count (and of the count block) and the wait.
--spec also times the NumPy restatement (tests/segment_spec.py) of the same frame on this machine's CPU.  The split into
kernels comes from a separate `rocprofv3 --kernel-trace --stats` run of this tool.
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from semantic_slam_amd import capi, synth  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--repeats", type=int, default=50)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--ks", default="4,16,64")
ap.add_argument("--spec", action="store_true")
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
    for _ in range(args.warmup):
        call()
    ms = []
    for _ in range(args.repeats):
        t0 = time.perf_counter()
        call()
        ms.append((time.perf_counter() - t0) * 1e3)
    return ms


def dilate(m, r):
    h, w = m.shape
    pad = np.zeros((h + 2 * r, w + 2 * r), bool)
    pad[r:r + h, r:r + w] = m
    out = np.zeros((h, w), bool)
    for dy in range(2 * r + 1):
        for dx in range(2 * r + 1):
            out |= pad[dy:dy + h, dx:dx + w]
    return out


H, W = synth.IM_H, synth.IM_W
scene = synth.ObjectScene()
pose = scene.pose(3)
depth, ids = scene.depth(pose), scene.ids(pose)
base = [np.where(dilate(ids == i, 6), 255, 0).astype(np.uint8) for i in range(len(scene.objects))]
p = capi.segment_params_default(capi.default_config(H, W))
d_depth = torch.from_numpy(depth).cuda()
d_don = torch.empty((H, W), dtype=torch.float32, device="cuda")
d_cl = torch.empty((H, W), dtype=torch.int32, device="cuda")
say(f"synth.ObjectScene() pose 3, {W}x{H}, defaults: radii {p.small_radius_m:g} / {p.large_radius_m:g} m, 2 x 289 taps per pixel")
with capi.Segmenter(H, W) as seg:
    n = seg.segment_depth(p, d_depth.data_ptr(), d_cl.data_ptr(), d_don.data_ptr())
    kept = int((d_cl > 0).sum().item())
    ms = timed(lambda: seg.segment_depth(p, d_depth.data_ptr(), d_cl.data_ptr(), d_don.data_ptr()))
    say(f"  tsdf_segment_depth_device (DoN image written), host clock around the call: {spread(ms)}; {n} clusters, "
        f"{kept} clustered pixels")
    for K in [int(x) for x in args.ks.split(",")]:
        km = torch.from_numpy(np.stack([base[j % len(base)] for j in range(K)])).cuda()
        ko = torch.empty_like(km)
        torch.cuda.synchronize()
        ms = timed(lambda: seg.refine_masks(p, d_cl.data_ptr(), n, km.data_ptr(), K, ko.data_ptr()))
        say(f"  K = {K:2d}: tsdf_segment_refine_masks_device (count block fetched): {spread(ms)}; "
            f"{int((ko == 255).sum().item())} refined of {int((km >= 128).sum().item())} mask pixels; "
            f"mask bytes read and written {2 * K * H * W / 1e6:.1f} MB")
        ms = timed(lambda: seg.segment_frame(p, d_depth.data_ptr(), km.data_ptr(), K, ko.data_ptr()))
        say(f"  K = {K:2d}: tsdf_segment_frame, host clock around the call: {spread(ms)}")

if args.spec:
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import segment_spec as ss  # noqa: E402
    sp = ss.from_ctypes(p)
    t0 = time.perf_counter()
    _, cl, c = ss.segment_depth(depth, sp)
    t1 = time.perf_counter()
    ss.refine(cl, c, np.stack(base), sp)
    t2 = time.perf_counter()
    say(f"  NumPy restatement on this machine's CPU: segment_depth {t1 - t0:.2f} s, refine (K = 4) {t2 - t1:.3f} s")

if args.out:
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
