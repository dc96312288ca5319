"""Times photometric tracking (tsdf_track_rgbd, csrc/tsdf_photo.hip.h) beside tsdf_track on the GPU.

    python tools/track_rgbd_time.py [--repeats 50] [--warmup 5] [--out FILE]

One 200^3 @ 3.84 mm TrackScene volume (two spheres and a wall) fused with colour from 16 frames of its orbit, one 640 x 480
frame of a held-out pose, the guess 1 deg / 1 cm off, default parameters.  Timed in turn, one call of each per round, so that
all of them see the same box at the same time:

  tsdf_track                     the frame already on the device
  tsdf_track_rgbd, no rgb        the same track from a host frame: the staging copy on top
  tsdf_track_rgbd, rgb           the combined track: the rgb copy, the live pyramid, the model pyramid, the photometric passes
  tsdf_raycast, depth only       the render into host memory ...
  tsdf_render_intensity, level 2 ... and with the model intensity kernel, both halvings and a level-2 copy instead of a
                                 level-0 one: the difference is what the model pyramid costs a track

Every call returns when its result is on the host, so a host clock around it is a timing of finished work.  The split by
kernel comes from a separate `rocprofv3 --kernel-trace --stats` run of this tool.
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
import photo_cases as pc  # noqa: E402
import track_spec as ts  # noqa: E402
from semantic_slam_amd import capi, synth  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--repeats", type=int, default=50)
ap.add_argument("--warmup", type=int, default=5)
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


E = 200
vs = 0.768 / E
origin = synth.surf_volume(E, vs, 0.8)
cfg = capi.make_config((E,) * 3, vs, origin)
scene = synth.TrackScene((E,) * 3, vs, origin)
with capi.Volume(cfg) as vol:
    vol.colour_enable()
    for k in range(0, 64, 4):
        c = scene.pose(k)
        d, rgb = pc.frame(scene, c)
        vol.integrate_rgbd(d, rgb, c)
    true = scene.pose(7)
    guess = ts.perturb(true, np.random.default_rng(5), 1.0, 0.01)
    depth, rgb = pc.frame(scene, true)
    d_dev = torch.from_numpy(depth).cuda()
    ray = capi.raycast_params_default(cfg)
    calls = {
        "tsdf_track": lambda: vol.track(d_dev.data_ptr(), guess),
        "tsdf_track_rgbd, no rgb": lambda: vol.track_rgbd(depth, None, guess),
        "tsdf_track_rgbd, rgb": lambda: vol.track_rgbd(depth, rgb, guess),
        "tsdf_raycast, depth only": lambda: vol.raycast(guess, params=ray, normals=False),
        "tsdf_render_intensity, level 2": lambda: vol.render_intensity(guess, level=2, params=ray),
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
    say(f"200^3 @ {vs * 1e3:.2f} mm TrackScene with colour, 640x480, defaults (photo_weight "
        f"{capi.photo_params_default(cfg).photo_weight:.3g}), one call of each per round:")
    for name in calls:
        say(f"  {name:32s} {spread(ms[name])}")
    for name in ("tsdf_track", "tsdf_track_rgbd, no rgb", "tsdf_track_rgbd, rgb"):
        pose, st = last[name]
        e = ts.pose_error(pose, true)
        say(f"  {name}: {st}; error {e[0]:.1e} m {e[1]:.1e} rad")
    assert last["tsdf_track"][0].tobytes() == last["tsdf_track_rgbd, no rgb"][0].tobytes()

if args.out:
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
