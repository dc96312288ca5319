"""The summary words across the one-frame launch sites the walks do not reach: the measurement build's (variant 11's masked
row-mapped launch and the ladder, with and without a summary: csrc/tsdf_experiments_host.hip.h), beside the product's masked
brick launch on the same script.  A 256 x 8 x 8 volume -- row-mapped, one segment per row, several workgroups -- takes an
integrate_tile launch (every word carries the count 1), the launch under test, and another integrate_tile launch, which takes
the weights from whatever words it meets; after each, every word is held to summary_spec's Predictor and must be sound for
the arrays, and the arrays equal the CPU oracle's bit for bit.  The measurement build's cases appear when it is the loaded
library (capi.variants).

Who reaches the other callers of summary_before (csrc/tsdf_capi.hip) -- the walks with every word predicted step by step, the
others with the arrays bit for bit against the reference or the oracle:
  launch_integrate, scalar kernel     test_gpu_walk.py (runs walks: masked_handover under variant 1), test_gpu_weight_runs.py
                                      (test_scalar_kernel_and_reset)
  launch_integrate, integrate_tile    test_gpu_walk.py (runs walks), test_gpu_weight_runs.py, test_gpu_run_division.py
  launch_masked_bricks                test_gpu_walk.py (masked_handover under variant 8; flat walks, through launch_multi),
                                      test_gpu_weight_runs.py (test_masked_brick_launch_forgets_the_runs)
  launch_multi                        test_gpu_walk.py (every fused step), test_gpu_weight_runs.py
                                      (test_fused_launch_forgets_the_runs), test_gpu_multiframe.py
  the batched launch, per member      test_gpu_walk.py (test_walk_batch_runs), test_gpu_batch.py"""
import numpy as np
import pytest

import summary_spec as ss
from semantic_slam_amd import capi, synth

pytestmark = pytest.mark.gpu

DIMS, VS = (256, 8, 8), 0.005
# (variant, masked, the Predictor's step); 23: ladder_tile without a summary, 39: with one
SITES = [(8, True, "forget"), (11, True, "forget"), (23, False, "drop"), (39, False, "forget")]


@pytest.mark.parametrize("variant,masked,step", [s for s in SITES if s[0] in capi.variants(*(v for v, _, _ in SITES))])
def test_words_after_the_launch(cuda, oracle, variant, masked, step):
    origin = synth.sband_volume(DIMS, VS)
    cfg = capi.make_config(DIMS, VS, origin, trunc=synth.SBAND_TRUNC)
    depth = synth.sfull_depth()
    mask = np.zeros(depth.shape, np.uint8)
    mask[:, :330] = 255                         # part of every row of voxels: the masked frame updates segments partly
    seen = depth * (mask >= 128) if masked else depth
    depth_dev, mask_dev = cuda.from_numpy(depth).cuda(), cuda.from_numpy(mask).cuda()
    lay = ss.Layout(DIMS)
    pred = ss.Predictor(lay)
    t, w = oracle.init_grid(DIMS)

    def model(frame, k):
        t0, w0 = t.copy(), w.copy()
        oracle.integrate(cfg.cam_K, oracle.cam2base(synth.identity_pose(), synth.sband_pose(k)), frame, DIMS, origin, VS, cfg.trunc_margin, t, w)
        pred.frame(t0, w0, t, w)

    def check(vol, what):
        got_t, got_w = vol.download()
        assert np.array_equal(got_w.view(np.uint32), w.view(np.uint32)), f"{what}: weights differ from the oracle"
        assert np.array_equal(got_t.view(np.uint32), t.view(np.uint32)), f"{what}: TSDF differs from the oracle"
        words = vol.summary_words()
        ss.assert_sound(lay, words, got_t, got_w, what)
        pred.check(words, what)

    with capi.Volume(cfg) as vol:
        vol.set_deferral(0)
        for k in range(3):
            under_test = k == 1
            vol.set_kernel_variant(variant if under_test else 0)
            model(seen if under_test else depth, k)
            if under_test and masked:
                vol.integrate_masked_device(depth_dev.data_ptr(), mask_dev.data_ptr(), synth.sband_pose(k))
            else:
                vol.integrate_device(depth_dev.data_ptr(), synth.sband_pose(k))
            if not under_test or variant in capi.SHIPPED_VARIANTS:
                pred.launches([("one", 0 if not under_test else variant)], [under_test and masked])
            else:                               # the measurement build's kernels: the step is stated here
                pred.frames.pop(0)
                getattr(pred, step)()
            check(vol, f"variant {variant}, launch {k}")
            if k == 0:
                assert np.all(vol.summary_words() == ss.FRESH & ~ss.ONES | (1 << ss.COUNT_SHIFT)), "S-band: every segment wholly updated once"
        assert pred.tile_launches == 2
        assert not ss.has_run(vol.summary_words()).any(), "no launch starts a run"
