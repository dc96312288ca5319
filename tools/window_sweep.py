"""Development probe (not a test, not the bench): ms per frame of the one-frame kernel (integrate_tile<2, false>, variant 3)
on the S-band workload for every Infinity Cache window size and head load policy.  Needs the
measurement build, whose knobs TSDF_MALL_WINDOW_MB / TSDF_SWEEP_FORWARD / TSDF_HEAD_PLAIN_LOADS are read per launch:
    make -C semantic_slam_amd/csrc experiments
    TSDF_HIP_LIB=$PWD/semantic_slam_amd/libtsdf_hip_exp.so python tools/window_sweep.py [grid] [frames] [rounds] [z_begin z_end]
(SWEEP_WINDOWS=32,64,... : the window sizes in MiB)"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from semantic_slam_amd import capi, synth  # noqa: E402

D = int(sys.argv[1]) if len(sys.argv) > 1 else 512
frames = int(sys.argv[2]) if len(sys.argv) > 2 else 256
rounds = int(sys.argv[3]) if len(sys.argv) > 3 else 3
zb, ze = (int(sys.argv[4]), int(sys.argv[5])) if len(sys.argv) > 5 else (0, D)
assert capi.experiments_build(), "needs the measurement build (TSDF_HIP_LIB=.../libtsdf_hip_exp.so)"
vs = {512: 0.005, 1024: 0.002}.get(D, 2.56 / D)
dims = (D, D, D)
cfg = capi.make_config(dims, vs, synth.sband_volume(dims, vs), trunc=synth.SBAND_TRUNC, z_begin=zb, z_end=ze)
poses = np.stack([synth.sband_pose(k) for k in range(frames)])
d = torch.from_numpy(synth.sfull_depth()).cuda()
state_mib = 8 * D * D * (ze - zb) / 2 ** 20

# (label, window MiB, always forward, head loads plain)
WINDOWS = [int(w) for w in os.environ.get("SWEEP_WINDOWS", "32,64,96,128,160,192,224,256").split(",")]
settings = [("forward, no window (as before)", 0, 1, 0), ("alternating, no window", 0, 0, 0)]
settings += [(f"window {w} MiB, head loads nt", w, 0, 0) for w in WINDOWS]
settings += [(f"window {w} MiB, head loads plain", w, 0, 1) for w in (64, 128, 192)]
settings += [(f"window {w} MiB, always forward", w, 1, 0) for w in (128, 1024)]

res = {s[0]: [] for s in settings}
with capi.Volume(cfg) as vol:
    vol.set_kernel_variant(3)
    for rnd in range(rounds):
        for label, w, fwd, head in settings:
            os.environ["TSDF_MALL_WINDOW_MB"] = str(w)
            os.environ["TSDF_SWEEP_FORWARD"] = str(fwd)
            os.environ["TSDF_HEAD_PLAIN_LOADS"] = str(head)
            vol.integrate_sequence_timed(d.data_ptr(), poses[:8])      # warm-up under this setting
            res[label].append(vol.integrate_sequence_timed(d.data_ptr(), poses) / frames)
print(f"S-band {D}x{D}x{D}, slab z [{zb}, {ze}) = {state_mib:.0f} MiB of state, {frames} frames per timed sequence, "
      f"{rounds} interleaved rounds; ms per frame: median (min .. max)")
for label, _, _, _ in settings:
    t = np.array(res[label])
    gbps = (16 * D * D * (ze - zb) + 4 * 480 * 640 + 100) / np.median(t) / 1e6
    print(f"  {label:36s} {np.median(t):.4f} ({t.min():.4f} .. {t.max():.4f})   {gbps:7.1f} GB/s at the 16 B model")
