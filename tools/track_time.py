"""Times frame-to-model tracking (tsdf_track, csrc/tsdf_track.hip.h) on the GPU.

    python tools/track_time.py [--repeats 50] [--warmup 5] [--only a,b,c] [--out FILE]

  (a) 512^3 @ 5 mm TrackScene (two spheres and a wall) fused from 32 frames of its orbit, 640 x 480, default parameters,
      guess 1 deg / 1 cm off a held-out pose;
  (b) the 1024^3 @ 2 mm fr3 trajectory volume (bench.py's traj composition, base = first keyframe, TrackScene instead of
      S-surf) fused from keyframes 0..31, tracked from keyframe 5 towards a pose 1/8 of the way to keyframe 6;
  (c) one 200^3 object volume (tsdf_batch member) with an instance mask.

Every call is timed with device events around it on a caller stream (tsdf_set_stream); the call ends with its own stream
synchronise, so the events bracket the render, the association and solve kernels and the result's copy.  The split into the
render and the association / solve kernels comes from a separate `rocprofv3 --kernel-trace --stats` run of this tool.  Also
printed: the convergence rate at raw keyframe steps of the golden fr3 poses (each keyframe tracked from the previous one).
"""
import argparse
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import track_spec as ts  # noqa: E402
from semantic_slam_amd import capi, ingest, synth  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--repeats", type=int, default=50)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--only", default="a,b,c")
ap.add_argument("--out", default="")
args = ap.parse_args()
which = set(args.only.split(","))
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def spread(ms):
    ms = np.sort(np.asarray(ms))
    return (f"median {np.median(ms):.4f} ms, min {ms[0]:.4f}, p10 {np.percentile(ms, 10):.4f}, p90 {np.percentile(ms, 90):.4f}, "
            f"max {ms[-1]:.4f} (n = {len(ms)})")


def time_track(vol, depth, guess, mask=None, p=None):
    s = torch.cuda.Stream()
    vol.set_stream(s.cuda_stream)
    ms, st = [], None
    for i in range(args.warmup + args.repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(s)
        _, st = vol.track(depth.data_ptr(), guess, params=p, mask_ptr=None if mask is None else mask.data_ptr())
        b.record(s)
        b.synchronize()
        if i >= args.warmup:
            ms.append(a.elapsed_time(b))
    vol.set_stream(None)
    return ms, st


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


if "a" in which:
    E, vs = 512, 0.005
    origin = synth.surf_volume(E, vs, 0.8)
    cfg = capi.make_config((E,) * 3, vs, origin)
    scene = synth.TrackScene((E,) * 3, vs, origin)
    with capi.Volume(cfg) as vol:
        poses = [scene.pose(k) for k in range(0, 64, 2)]
        frames = [dev(scene.depth(c, quantize=True)) for c in poses]
        vol.integrate_frames_device([d.data_ptr() for d in frames], np.stack(poses))
        true = scene.pose(9)
        guess = ts.perturb(true, np.random.default_rng(0), 1.0, 0.01)
        ms, st = time_track(vol, dev(scene.depth(true, quantize=True)), guess)
        got, _ = vol.track(dev(scene.depth(true, quantize=True)).data_ptr(), guess)
        e = ts.pose_error(got, true)
        say(f"(a) 512^3 @ 5 mm TrackScene, 640x480, defaults: {spread(ms)}; {st}; error {e[0]:.1e} m {e[1]:.1e} rad")

gold = np.load(os.path.join(ROOT, "tests", "golden", "fr3_office_keyframes.npz"), allow_pickle=False)
Twc = ingest.pose_inverse(gold["Tcw"])

if "b" in which:
    E, vs = 1024, 0.002
    base = Twc[0].ravel().astype(np.float32)
    half = E * vs / 2.0
    origin = np.array([-half, -half, 0.6], np.float32)
    cfg = capi.make_config((E,) * 3, vs, origin, base2world=base)
    scene = synth.TrackScene((E,) * 3, vs, origin)
    binv = capi.invert_matrix(base)[1]
    with capi.Volume(cfg) as vol:
        poses = [Twc[i].ravel().astype(np.float32) for i in range(32)]
        for k in range(0, 32, 8):
            frames = [dev(scene.depth(capi.multiply_matrix(binv, c), quantize=True)) for c in poses[k:k + 8]]
            vol.integrate_frames_device([d.data_ptr() for d in frames], np.stack(poses[k:k + 8]))
            vol.sync()
        T5, T6 = Twc[5].astype(np.float64), Twc[6].astype(np.float64)
        true = T5.copy()
        true[:3, 3] = T5[:3, 3] + (T6[:3, 3] - T5[:3, 3]) / 8
        true = true.astype(np.float32).ravel()
        live = dev(scene.depth(capi.multiply_matrix(binv, true), quantize=True))
        ms, st = time_track(vol, live, poses[5])
        say(f"(b) 1024^3 @ 2 mm fr3 trajectory volume, 640x480, defaults: {spread(ms)}; {st}")
        # convergence at raw keyframe steps, each keyframe tracked from the previous one (the golden poses' own motion)
        ok, n, errs = 0, 0, []
        for i in range(1, 32):
            live = dev(scene.depth(capi.multiply_matrix(binv, poses[i]), quantize=True))
            got, st = vol.track(live.data_ptr(), poses[i - 1])
            e = ts.pose_error(got, poses[i])
            d = ts.pose_error(poses[i - 1], poses[i])
            n += 1
            conv = st["status"] != 2 and e[0] < 0.01 and e[1] < math.radians(0.5)
            ok += conv
            errs.append((d[0], math.degrees(d[1]), conv))
        steps = np.array([(a, b) for a, b, _ in errs])
        say(f"(b) raw keyframe steps 1..31 (median {np.median(steps[:, 0]) * 100:.1f} cm / {np.median(steps[:, 1]):.1f} deg, "
            f"p90 {np.percentile(steps[:, 0], 90) * 100:.1f} cm / {np.percentile(steps[:, 1], 90):.1f} deg): "
            f"{ok} of {n} within 1 cm / 0.5 deg of the keyframe pose")
        say("    per step (cm, deg, converged): " + ", ".join(f"{a * 100:.1f}/{b:.1f}/{int(c)}" for a, b, c in errs))

if "c" in which:
    E = 200
    vs = 0.768 / E
    origin = synth.surf_volume(E, vs, 0.8)
    scene = synth.TrackScene((E,) * 3, vs, origin)
    cfg = capi.make_config((E,) * 3, vs, origin)
    mask = np.zeros((480, 640), np.uint8)
    mask[90:400, 120:540] = 255
    m = dev(mask)
    with capi.Batch([cfg]) as batch:
        for k in range(0, 64, 4):
            c = scene.pose(k)
            batch.integrate_device(dev(scene.depth(c, quantize=True)).data_ptr(), [m.data_ptr()], c)
        batch.sync()
        vol = batch.volumes[0]
        true = scene.pose(7)
        guess = ts.perturb(true, np.random.default_rng(5), 1.0, 0.01)
        ms, st = time_track(vol, dev(scene.depth(true, quantize=True)), guess, mask=m)
        say(f"(c) 200^3 object (batch member) with its mask, 640x480, defaults: {spread(ms)}; {st}")

if args.out:
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
