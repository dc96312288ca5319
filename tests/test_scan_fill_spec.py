"""The gap-fill restatement (tests/scan_fill_spec.py) on the CPU: every named case of tests/scan_fill_cases.py reaches the
branch it is named for (the cases assert that as they are built), a second, pixel-by-pixel statement of the rule gives the
same bits, planes come out to rounding, and the KITTI-sized scan gains the surface the sparse image lacks.
tests/test_gpu_scan_fill.py holds the device to the same images."""
import os
import re

import numpy as np
import pytest

import scan_cases
import scan_fill_cases as cases
import scan_fill_spec as spec
from semantic_slam_amd import synth

F = np.float32
EPS = 2.0 ** -24


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def test_every_case_is_there():
    names = [c["name"] for c in cases.small_cases()]
    assert len(names) == len(set(names)) and len(names) > 30
    for want in ("spans_0_0_identity", "spans_1_1_identity", "distance_u_span_5", "distance_v_span_16", "nearer_source_wins",
                 "one_side_only", "row_does_not_wrap", "image_borders", "jump_exact_and_one_ulp_above",
                 "two_against_three_at_default_jump", "v_pass_fed_by_u_filled", "v_pass_not_fed_by_v_filled",
                 "non_sources_keep_their_bits", "flt_max_and_denormal_sources", "pairs_across_tile_borders", "sparse_130x131_spans_16_16",
                 "all_empty", "all_measured", "sparse_1x300_spans_5_8", "sparse_300x1_spans_5_8", "sparse_8x64_spans_16_16"):
        assert want in names, want
    assert {(c["H"], c["W"]) for c in cases.small_cases()} == set(cases.SHAPES)
    for c in cases.small_cases():
        k, d, f = c["kind"], c["depth"], c["filled"]
        assert f.dtype == F and k.dtype == np.uint8 and f.shape == d.shape == k.shape
        assert c["n_filled"] == np.count_nonzero(k >= 2)
        assert np.array_equal(bits(f)[k <= 1], bits(d)[k <= 1])          # measured and empty pixels keep their bits
        assert np.all(spec.is_source(f[k >= 1])) and not np.any(spec.is_source(f[k == 0]))


def test_the_cases_straddle_the_header_s_tile():
    """The cases import nothing of the library: their tile and span constants are the header's, read from its text."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "semantic_slam_amd", "csrc", "tsdf_scan_fill.hip.h")) as f:
        text = f.read()
    m = re.search(r"constexpr int kFillTileW = (\d+), kFillTileH = (\d+);", text)
    assert m and (int(m.group(1)), int(m.group(2))) == (cases.TILE_W, cases.TILE_H)
    m = re.search(r"constexpr int kFillMaxSpan = (\d+),", text)
    assert m and int(m.group(1)) == spec.MAX_SPAN
    assert (cases.TILE_H, cases.TILE_W) in cases.SHAPES
    assert any(h > 2 * cases.TILE_H and w > 2 * cases.TILE_W and h % cases.TILE_H and w % cases.TILE_W for h, w in cases.SHAPES)


def test_default_parameters_and_their_range():
    assert spec.DEFAULT == (5, 8, F(0.05)) and spec.params_ok(*spec.DEFAULT)
    assert spec.params_ok(0, 0, 0.0) and spec.params_ok(16, 16, 1e30)
    for bad in ((-1, 8, 0.05), (5, 17, 0.05), (5, 8, -0.01), (5, 8, np.nan), (5, 8, np.inf), (17, 0, 0.0)):
        assert not spec.params_ok(*bad), bad


def test_scalar_restatement_equals_the_vectorised_one_on_every_small_case():
    for c in cases.small_cases():
        f, k, n = spec.fill_scalar(c["depth"], *c["params"])
        assert np.array_equal(bits(f), bits(c["filled"])), c["name"]
        assert np.array_equal(k, c["kind"]) and n == c["n_filled"], c["name"]


def test_scalar_restatement_on_random_cases():
    for seed in range(20):
        c = cases.random_case(seed)
        f, k, n = spec.fill_scalar(c["depth"], *c["params"])
        assert np.array_equal(bits(f), bits(c["filled"])) and np.array_equal(k, c["kind"]) and n == c["n_filled"], c["name"]


def test_scalar_restatement_on_rows_of_the_kitti_case():
    c = cases.kitti_case()
    for rows in ((170, 190), (0, 3), (370, 375)):             # a band across the measured rows, and the image's first and last
        f, k, _ = spec.fill_scalar(c["depth"], *c["params"], rows=rows)
        assert np.array_equal(bits(f), bits(c["filled"][rows[0]:rows[1]])), rows
        assert np.array_equal(k, c["kind"][rows[0]:rows[1]]), rows
    assert np.count_nonzero(c["kind"][170:190] == 2) > 100 and np.count_nonzero(c["kind"][170:190] == 3) > 100


def test_planes_come_out_to_rounding():
    """A plane's inverse z-depth is affine in the pixel: 1 / z = alpha + beta u + gamma v.  Sampled on a sparse lattice and
    filled with jump_rel huge, every filled pixel is the plane to the roundings on its path: input, reciprocal, product, sum,
    quotient, reciprocal for the u pass (6), and from the second reciprocal on once more for the v pass (11)."""
    rng = np.random.default_rng(42)
    h, w = 40, 56
    v, u = np.mgrid[0:h, 0:w].astype(np.float64)
    worst = {2: 0.0, 3: 0.0}
    for _ in range(300):
        su, sv = int(rng.integers(2, 17)), int(rng.integers(2, 17))
        alpha = rng.uniform(0.05, 1.0)
        beta, gamma = rng.uniform(-1, 1, 2) * alpha * 0.9 / (w + h)            # 1 / z stays positive over the image
        z = 1.0 / (alpha + beta * u + gamma * v)
        sparse = np.zeros((h, w), F)
        ou, ov = int(rng.integers(0, su)), int(rng.integers(0, sv))
        sparse[ov::sv, ou::su] = z[ov::sv, ou::su].astype(F)
        f, k, n = spec.fill(sparse, su, sv, F(1e30))
        assert n > 0
        rel = np.abs(f.astype(np.float64) - z) / z
        for kind, bound in ((2, 6), (3, 11)):
            if np.any(k == kind):
                worst[kind] = max(worst[kind], float(rel[k == kind].max()) / EPS)
                assert rel[k == kind].max() <= bound * EPS, (kind, rel[k == kind].max() / EPS)
        # the lattice is closed: every pixel inside the outermost samples is written
        inner = k[ov:ov + (h - 1 - ov) // sv * sv + 1, ou:ou + (w - 1 - ou) // su * su + 1]
        assert np.all(inner >= 1)
    print(f"planes: worst relative error {worst[2]:.2f} eps (u pass), {worst[3]:.2f} eps (v pass), eps = 2^-24")


@pytest.fixture(scope="module")
def kitti_fusion(oracle):
    """(updated, band) voxels of the oracle for the sparse and for the filled depth image of the calibration scan."""
    c = cases.kitti_case()
    scene = scan_cases.kitti_scene()
    pose = scene.pose(0, n=16, max_yaw_deg=5.0)
    K = scan_cases.calibration_case()["K"]
    trunc = float(F(scene.vs) * F(5))
    out = {}
    for name, depth in (("sparse", c["depth"]), ("filled", c["filled"])):
        t, w = oracle.init_grid(scene.dims)
        oracle.integrate(K, oracle.cam2base(synth.identity_pose(), pose), depth, scene.dims, scene.origin.astype(F), scene.vs, trunc,
                         t, w, max_depth=80.0)
        out[name] = (int(np.count_nonzero(w)), int(np.count_nonzero((w > 0) & (np.abs(t) < 1))))
    return out


def test_kitti_case_with_the_default_parameters(kitti_fusion):
    c = cases.kitti_case()
    k = c["kind"]
    n_px = k.size
    print(f"kitti: {np.count_nonzero(k == 1)} measured, {np.count_nonzero(k == 2)} u-filled, {np.count_nonzero(k == 3)} v-filled of "
          f"{n_px} pixels ({100.0 * np.count_nonzero(k) / n_px:.1f} % written); fused: {kitti_fusion}")
    assert c["params"] == (5, 8, float(F(0.05)))
    assert c["n_filled"] > 150000
    rows = np.flatnonzero((k == 1).any(axis=1))
    cols = np.flatnonzero((k == 1).any(axis=0))
    assert not np.any(k[:rows[0]] >= 2) and not np.any(k[rows[-1] + 1:] >= 2)          # nothing beyond the outermost beams
    assert not np.any(k[:, :cols[0]] >= 2) and not np.any(k[:, cols[-1] + 1:] >= 2)
    (upd_s, band_s), (upd_f, band_f) = kitti_fusion["sparse"], kitti_fusion["filled"]
    assert upd_s > 1000 and band_s > 1000
    assert upd_f >= 10 * upd_s, (upd_f, upd_s)
    assert band_f >= 10 * band_s, (band_f, band_s)
