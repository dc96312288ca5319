"""Times joint tracking against a batch (tsdf_batch_track, csrc/tsdf_batch_track.hip.h) on the GPU, against what a caller
of an object map does without it: one tsdf_track_system per member on the borrowed handles, each with its object's mask
(one render, one association pass and one host wait per member, for the systems of ONE iteration).

    python tools/batch_track_time.py [--repeats 50] [--warmup 5] [--only a,b] [--out FILE]

  (a) 16 members of 200^3 @ 4 mm placed over a TrackScene (two spheres and a wall), each fed depth x its instance mask (a
      0.5 m box around its centre, tools/batch_time.py's layout), 640 x 480, default parameters, guess 1 deg / 1 cm off a
      held-out pose;
  (b) synth.ObjectScene's four objects as members of different grids (the product case of tests/test_gpu_batch_track.py),
      cos 40 deg, min_inliers 100.

Every figure is host wall-clock around calls that end with their own stream wait (the render alone is followed by
tsdf_batch_sync), from the same run.  The split: render = tsdf_batch_raycast_device; member pass = a call with no iterations
(render + init + member pass) minus the render; iterations = the full call minus the call with no iterations.
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
import batch_track_cases as bc  # noqa: E402
import track_spec as ts  # noqa: E402
from semantic_slam_amd import capi, synth  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--repeats", type=int, default=50)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--only", default="a,b")
ap.add_argument("--out", default="")
args = ap.parse_args()
which = set(args.only.split(","))
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def spread(ms):
    ms = np.sort(np.asarray(ms))
    return f"median {np.median(ms):.4f} ms, p10 {np.percentile(ms, 10):.4f}, p90 {np.percentile(ms, 90):.4f} (n = {len(ms)})"


def timed(fn):
    ms, out = [], None
    for i in range(args.warmup + args.repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        dt = (time.perf_counter() - t0) * 1e3
        if i >= args.warmup:
            ms.append(dt)
    return ms, out


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def measure(name, batch, p, live, masks, guess, true):
    """The table of one batch: live a device frame, masks one device mask per member (today's way needs them)."""
    M = len(batch.cfgs)
    px = p.ray.im_height * p.ray.im_width
    rd, rn, rm = (torch.empty(px, dtype=torch.float32, device="cuda"), torch.empty(3 * px, dtype=torch.float32, device="cuda"),
                  torch.empty(px, dtype=torch.int32, device="cuda"))
    none = capi.TrackParams.from_buffer_copy(p)
    none.iters[:] = (0, 0, 0)

    def render():
        batch.raycast_device(guess, rd.data_ptr(), rn.data_ptr(), rm.data_ptr(), params=p.ray)
        batch.sync()

    def today():
        return [v.track_system(live.data_ptr(), guess, guess, level=0, params=p, mask_ptr=m.data_ptr())
                for v, m in zip(batch.volumes, masks)]

    t_full, (pose, st, systems) = timed(lambda: batch.track(live.data_ptr(), guess, params=p))
    t_nosys, _ = timed(lambda: batch.track(live.data_ptr(), guess, params=p, want_systems=False))
    t_none, _ = timed(lambda: batch.track(live.data_ptr(), guess, params=none))
    t_sys, _ = timed(lambda: batch.track_system(live.data_ptr(), guess, guess, level=0, params=p))
    t_render, _ = timed(render)
    t_today, _ = timed(today)
    e = ts.pose_error(pose, true)
    iters = sum(st["iters_run"])
    med = lambda x: float(np.median(x))  # noqa: E731
    say(f"({name}) {M} members, {p.ray.im_width}x{p.ray.im_height}: {st}; error {e[0]:.1e} m {e[1]:.1e} rad; "
        f"member pairs {systems[:, 28].astype(int).tolist()}")
    say(f"    tsdf_batch_track with systems ({sum(p.iters)} iterations queued, {iters} run): {spread(t_full)}")
    say(f"    tsdf_batch_track, member_systems NULL:                       {spread(t_nosys)}")
    say(f"    tsdf_batch_track_system (render + one member pass):          {spread(t_sys)}")
    say(f"    today: {M} x tsdf_track_system on the borrowed handles, masks: {spread(t_today)}")
    say(f"    split of the full call (medians): render {med(t_render):.4f} ms, member pass {med(t_none) - med(t_render):.4f} ms, "
        f"iterations {med(t_full) - med(t_none):.4f} ms ({(med(t_full) - med(t_none)) / max(sum(p.iters), 1):.4f} ms per queued iteration)")
    say(f"    one call for all members against {M} calls for one iteration's systems: x{med(t_today) / med(t_sys):.2f} "
        f"(tsdf_batch_track_system), x{med(t_today) / med(t_full):.2f} (the whole track, {iters} iterations and the member pass)")


if "a" in which:
    n, E = 16, 200
    vs = 0.8 / E
    rng = np.random.default_rng(0)
    K = synth.TUM_K
    cfgs, masks = [], []
    for i in range(n):
        o = np.array([-0.4 + rng.uniform(-0.3, 0.3), -0.4 + rng.uniform(-0.25, 0.25), 0.7 + rng.uniform(0, 0.8)], np.float32)
        cfgs.append(capi.make_config((E, E, E), vs, o, vol_id=i))
        c = o + 0.4
        u0, u1 = K[0] * (c[0] - 0.25) / c[2] + K[2], K[0] * (c[0] + 0.25) / c[2] + K[2]
        v0, v1 = K[4] * (c[1] - 0.25) / c[2] + K[5], K[4] * (c[1] + 0.25) / c[2] + K[5]
        m = np.zeros((480, 640), np.uint8)
        m[max(0, int(v0)):max(0, min(480, int(v1))), max(0, int(u0)):max(0, min(640, int(u1)))] = 255
        masks.append(dev(m))
    scene = synth.TrackScene((E, E, E), 0.004, np.array([-0.4, -0.4, 0.7], np.float32))
    with capi.Batch(cfgs) as batch:
        keep = []
        for k in range(0, 64, 4):
            c = scene.pose(k)
            keep.append(dev(scene.depth(c, quantize=True)))
            torch.cuda.synchronize()
            batch.integrate_device(keep[-1].data_ptr(), [m.data_ptr() for m in masks], c)
        batch.sync()
        true = scene.pose(7)
        guess = ts.perturb(true, np.random.default_rng(5), 1.0, 0.01)
        measure("a", batch, capi.track_params_default(cfgs[0]), dev(scene.depth(true, quantize=True)), masks, guess, true)

if "b" in which:
    scene, true, live, _ = bc.frames(1)
    cfgs = []
    voxels = (0.006, 0.008, 0.005, 0.007)
    for i in range(len(synth.OBJECTS)):
        lo, hi = scene.bounds(i)
        lo = lo - 0.06
        dims = np.ceil((hi + 0.06 - lo) / voxels[i]).astype(int) + 1
        dims[0] = (dims[0] + 3) // 4 * 4
        cfgs.append(capi.make_config(tuple(int(x) for x in dims), voxels[i], lo.astype(np.float32), vol_id=i))
    with capi.Batch(cfgs) as batch:
        keep = []
        for k in range(0, 16, 2):
            c = scene.pose(k)
            ids = scene.ids(c)
            keep.append((dev(scene.depth(c)), [dev(np.where(ids == o, 255, 0).astype(np.uint8)) for o in range(len(cfgs))]))
            torch.cuda.synchronize()
            batch.integrate_device(keep[-1][0].data_ptr(), [m.data_ptr() for m in keep[-1][1]], c)
        batch.sync()
        p = capi.track_params_default(cfgs[0])
        p.cos_normal_thresh, p.min_inliers = bc.COS_WIDE, bc.MIN_INLIERS
        ids = scene.ids(true)
        masks = [dev(np.where(ids == o, 255, 0).astype(np.uint8)) for o in range(len(cfgs))]
        measure("b", batch, p, dev(live), masks, bc.guess_of(true, bc.CANDIDATE_SEEDS[0]), true)

if args.out:
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
