"""The CPU restatement against the reference's own GpuIntegrate body compiled for the host
(oracle/_ref, `make -C oracle ref`; exists only where the reference was present at build time).
Random grids, poses and depth images: bit-exact.  What the reference body returned on these inputs is
stored (tests/golden/ref_oracle_vs_ref.npz, digests of its TSDF and weights), so the comparison runs
everywhere; where oracle/_ref exists the body is also run live and checked against both."""
import numpy as np
import pytest

from oracle.oracle import Ref
from ref_vectors import Stored, digest
from semantic_slam_amd import synth


@pytest.fixture(scope="module")
def stored():
    return Stored("oracle_vs_ref")


def _run(impl, K, c2bs, depths, dims, origin, vs, trunc, threads=0):
    """(tsdf, weight) of a fresh grid after impl (Oracle or Ref) integrated the frames in order."""
    from oracle.oracle import Oracle
    t, w = Oracle().init_grid(dims)
    for c2b, depth in zip(c2bs, depths):
        impl.integrate(K, c2b, depth, dims, origin, vs, trunc, t, w, threads=threads)
    return t, w


def _compare(stored, key, oracle, inputs, run_args, threads):
    """The oracle's result against the stored reference result, and, where it was built, against the live reference."""
    stored.check_inputs(key, *inputs)
    t1, w1 = _run(oracle, *run_args, threads=threads[0])
    if Ref.available():
        t2, w2 = _run(Ref(), *run_args, threads=threads[1])
        assert digest(t2, w2) == stored.str(key), f"{key}: the live reference differs from its stored result"
        assert np.array_equal(w1, w2)
        assert np.array_equal(t1.view(np.uint32), t2.view(np.uint32))
    assert digest(t1, w1) == stored.str(key), f"{key}: the oracle differs from the reference's stored result"
    return t1, w1


def body_case(oracle, seed):
    """Inputs of test_oracle_equals_reference_body: (K, cam2base poses, depth frames, dims, origin, voxel size, trunc)."""
    rng = np.random.default_rng(seed)
    dims = tuple(int(x) for x in rng.integers(8, 60, 3))
    vs = float(rng.choice([0.004, 0.01, 0.02, 0.05]))
    trunc = float(np.float32(vs) * np.float32(5))
    origin = synth.surf_volume(max(dims), vs, z0=float(rng.uniform(-0.2, 2.0)))
    h, w = int(rng.integers(30, 120)), int(rng.integers(40, 160))
    K = np.array([rng.uniform(50, 150), 0, w / 2 + rng.uniform(-3, 3), 0, rng.uniform(50, 150),
                  h / 2 + rng.uniform(-3, 3), 0, 0, 1], np.float32)
    sc = synth.SurfScene(dims, vs, origin, K=K, h=h, w=w)
    c2bs, depths = [], []
    for k in range(4):
        base = synth.identity_pose() if seed % 2 == 0 else synth.random_pose(rng)
        c2b = oracle.cam2base(base, synth.random_pose(rng, 0.5, 0.5))
        depth = sc.depth(c2b, quantize=bool(k & 1))
        depth[rng.integers(0, h, 40), rng.integers(0, w, 40)] = rng.choice([0.0, -1.0, 6.5, 6.0], 40)
        c2bs.append(c2b)
        depths.append(depth)
    return K, c2bs, depths, dims, origin, vs, trunc


def case_inputs(K, c2bs, depths, dims, origin, vs, trunc):
    return [K, np.stack(c2bs), np.stack(depths), np.array(dims), np.asarray(origin), np.array([vs, trunc])]


DEGENERATE_DIMS, DEGENERATE_VS, DEGENERATE_TRUNC = (12, 12, 12), 0.05, 0.25


def degenerate_cases():
    """Inputs of test_degenerate_poses_match, one (K, [cam2base], [depth], dims, origin, voxel size, trunc) per pose."""
    origin = np.array([-0.3, -0.3, -0.3], np.float32)
    depth = np.full((48, 64), 1.0, np.float32)
    K = np.array([50, 0, 32, 0, 50, 24, 0, 0, 1], np.float32)
    return [(K, [c2b], [depth], DEGENERATE_DIMS, origin, DEGENERATE_VS, DEGENERATE_TRUNC)
            for c2b in (np.zeros(16, np.float32),
                        synth.make_pose(np.eye(3) * 1e-30, [0, 0, 0]),
                        synth.make_pose(np.eye(3) * 1e30, [0, 0, 0]),
                        synth.make_pose(np.eye(3), [0, 0, 1e20]))]


def non_finite_case():
    """Inputs of test_non_finite_depth_samples_match."""
    rng = np.random.default_rng(11)
    dims, vs = (40, 36, 30), 0.02
    origin = synth.surf_volume(max(dims), vs, 0.6)
    sc = synth.SurfScene(dims, vs, origin)
    odd = np.array([np.nan, np.inf, -np.inf, -0.0, 1e-42, -1e-42, 6.0, np.nextafter(np.float32(6.0), np.float32(7.0))], np.float32)
    c2bs, depths = [], []
    for k in range(4):
        c2b = sc.pose(k, 8)
        depth = sc.depth(c2b, quantize=True)
        depth[rng.integers(0, 480, 20000), rng.integers(0, 640, 20000)] = rng.choice(odd, 20000)
        c2bs.append(c2b)
        depths.append(depth)
    return synth.TUM_K, c2bs, depths, dims, origin, vs, 0.1


@pytest.mark.parametrize("seed", range(8))
def test_oracle_equals_reference_body(oracle, stored, seed):
    case = body_case(oracle, seed)
    _compare(stored, f"body{seed}", oracle, case_inputs(*case), case, threads=(3, 2))


def test_degenerate_poses_match(oracle, stored):
    """Singular / huge / tiny pose entries: both sides take the same branches, no crash."""
    for i, case in enumerate(degenerate_cases()):
        _compare(stored, f"degenerate{i}", oracle, case_inputs(*case), case, threads=(0, 0))


def test_non_finite_depth_samples_match(oracle, stored):
    """NaN passes both of the reference's depth tests (ref: src/tsdf.cu:46,49 -- every comparison with NaN is false)
    and updates the voxel with dist = fmin(1, NaN) = 1; +-inf, negative and denormal samples take the ordinary
    branches.  The restatement must do exactly the same."""
    case = non_finite_case()
    t1, w1 = _compare(stored, "non_finite", oracle, case_inputs(*case), case, threads=(3, 2))
    assert np.isfinite(t1).all() and w1.max() >= 3
