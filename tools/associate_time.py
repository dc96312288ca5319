"""Times instance association (tsdf_batch_associate, csrc/tsdf_associate.hip.h) on the GPU.

    python tools/associate_time.py [--repeats 50] [--warmup 5] [--ks 4,16,64] [--out FILE]

The batch of tools/batch_time.py: 16 object volumes of 200^3 @ 4 mm with instance masks, 40 masked frames fused; the live
frame and the render at a held-out pose of its orbit, 640 x 480.  K instance masks are the batch's 16 box masks, repeated to
K.  Per K: the whole call (host clock around it; the call ends with its own stream synchronise, so the time covers the
collected-frame check, the render, the zeroing of the block, the counting kernel, the block's copy and the host assignment),
and the batch render alone (tsdf_batch_raycast_device + tsdf_batch_sync) for comparison.  The split into the render and the
counting kernel comes from a separate `rocprofv3 --kernel-trace --stats` run of this tool.
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
ap.add_argument("--ks", default="4,16,64")
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


# the batch of tools/batch_time.py (--n 16 --edge 200 --masks instance)
n, E = 16, 200
rng = np.random.default_rng(0)
vs = 0.8 / E
K_cam = synth.TUM_K
cfgs, masks = [], []
for i in range(n):
    o = np.array([-0.4 + rng.uniform(-0.3, 0.3), -0.4 + rng.uniform(-0.25, 0.25), 0.7 + rng.uniform(0, 0.8)], np.float32)
    cfgs.append(capi.make_config((E, E, E), vs, o, vol_id=i))
    m = np.zeros((480, 640), np.uint8)
    c = o + 0.4
    u0, u1 = K_cam[0] * (c[0] - 0.25) / c[2] + K_cam[2], K_cam[0] * (c[0] + 0.25) / c[2] + K_cam[2]
    v0, v1 = K_cam[4] * (c[1] - 0.25) / c[2] + K_cam[5], K_cam[4] * (c[1] + 0.25) / c[2] + K_cam[5]
    m[max(0, int(v0)):max(0, min(480, int(v1))), max(0, int(u0)):max(0, min(640, int(u1)))] = 255
    masks.append(m)
scene = synth.SurfScene((200, 200, 200), 0.004, np.array([-0.4, -0.4, 0.7], np.float32))
poses = [scene.pose(k, 8) for k in range(8)]
depth = torch.from_numpy(scene.depth(poses[0])).cuda()
m_dev = [torch.from_numpy(m).cuda() for m in masks]
view = scene.pose(3, 8)
live = torch.from_numpy(scene.depth(view)).cuda()
say(f"{n} volumes of {E}^3 @ {vs * 1e3:.0f} mm, 40 masked frames fused; live frame and render at a held-out pose, 640x480")
with capi.Batch(cfgs) as batch:
    for k in range(40):
        batch.integrate_device(depth.data_ptr(), [m.data_ptr() for m in m_dev], poses[k % 8])
    batch.sync()
    p = capi.associate_params_default(cfgs[0])
    d = torch.empty((480, 640), dtype=torch.float32, device="cuda")
    who = torch.empty((480, 640), dtype=torch.int32, device="cuda")
    for _ in range(args.warmup):
        batch.raycast_device(view, d.data_ptr(), None, who.data_ptr(), params=p.ray)
    batch.sync()
    ms = []
    for _ in range(args.repeats):
        t0 = time.perf_counter()
        batch.raycast_device(view, d.data_ptr(), None, who.data_ptr(), params=p.ray)
        batch.sync()
        ms.append((time.perf_counter() - t0) * 1e3)
    say(f"  render alone (tsdf_batch_raycast_device depth + member, host clock around call + sync): {spread(ms)}")
    for K in [int(x) for x in args.ks.split(",")]:
        km = torch.from_numpy(np.stack([masks[j % n] for j in range(K)])).cuda()
        torch.cuda.synchronize()
        for _ in range(args.warmup):
            out = batch.associate(view, live.data_ptr(), km.data_ptr(), K, params=p)
        ms = []
        for _ in range(args.repeats):
            t0 = time.perf_counter()
            out = batch.associate(view, live.data_ptr(), km.data_ptr(), K, params=p)
            ms.append((time.perf_counter() - t0) * 1e3)
        assigned = int((out["assign"] >= 0).sum())
        say(f"  K = {K:2d}: tsdf_batch_associate, host clock around the call: {spread(ms)}; {assigned} of {K} masks assigned, "
            f"{int(out['member'][:, :3].sum())} rendered pixels with valid live depth, "
            f"{int(out['mask'][:, 0].sum())} mask pixels; mask bytes read {K * 480 * 640 / 1e6:.1f} MB")

if args.out:
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
