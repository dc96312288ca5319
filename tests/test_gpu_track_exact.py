"""Tracking on the device held to its rule (csrc/tsdf_track.hip.h) per pair, per iteration and per result field, against
tests/track_spec.py over the cases of tests/track_cases.py:

  * the system of a single pair (a mask on its three pixels) equals the double value of the restatement's float32 terms;
  * a system of n pairs is within n * 2^-52 * sum |term| per entry, its count exact (two double sums of the same terms);
  * a track's status, iters_run and inliers are the restatement's, its rmse and every entry of its pose within one float32 ulp
    (a lost track: the guess's own bits), in cases the CPU tests show to keep clear of the restatement's own thresholds.

Families: (a) value edges of the live frame and mask, (b) relative poses that put points behind the camera or off the image,
(c) a model rendered from a volume of value edges, (d) images too small for a level to have a sample, (e) the sizes where
the reduction changes lane, wave, workgroup or trip of the grid-stride loop, (f) the level state machine, (g) one handle
used for one size after another.  The model the restatement sees is the device's own render (bit-exact with raycast_spec,
test_gpu_raycast.py)."""
import numpy as np
import pytest

import track_cases as tc
import track_spec as ts
from test_gpu_raycast import edge_state
from test_gpu_track import fused_volume
from semantic_slam_amd import capi

pytestmark = pytest.mark.gpu

f32 = np.float32


class Rig:
    """The two volumes, the World over the device's renders, and the device calls of a Case."""

    def __init__(self, torch):
        self.torch = torch
        self.vol, self.cfg, origin = fused_volume(torch, tc.DIMS, tc.VS, z0=tc.Z0, poses_k=tc.FUSED_POSES)
        self.state = self.vol.download()
        self.edge = capi.Volume(self.cfg)
        self.edge.upload(*edge_state(tc.DIMS, np.random.default_rng(tc.EDGE_SEED)))
        self.vols = {"scene": self.vol, "edge": self.edge}
        self.world = tc.World(tc.DIMS, tc.VS, origin, self.render)

    def render(self, volume, ray, pose):
        o = self.vols[volume].raycast(pose, params=ray, normals=True)
        return o["depth"], o["normal"]

    def fresh(self):
        """A new handle with the fused volume's state: no scratch block yet."""
        v = capi.Volume(self.cfg)
        v.upload(*self.state)
        return v

    def dev(self, a):
        return None if a is None else self.torch.from_numpy(np.array(a, order="C")).cuda()    # a copy: renders are read-only

    def system(self, case, vol=None):
        """The 29 sums of tsdf_track_system."""
        d, m = self.dev(case.live), self.dev(case.mask)
        vol = vol or self.vols[case.volume]
        A, b, r2, n = vol.track_system(d.data_ptr(), case.ref, case.cur, level=case.level, params=case.params(),
                                       mask_ptr=None if m is None else m.data_ptr())
        return np.concatenate([A[np.triu_indices(6)], b, [r2, float(n)]])

    def track(self, case, vol=None):
        d, m = self.dev(case.live), self.dev(case.mask)
        return (vol or self.vols[case.volume]).track(d.data_ptr(), case.ref, params=case.params(),
                                                     mask_ptr=None if m is None else m.data_ptr())

    def close(self):
        self.vol.close()
        self.edge.close()


@pytest.fixture(scope="module")
def rig(cuda):
    r = Rig(cuda)
    yield r
    r.close()


def check_system(rig, case, min_pairs=0):
    """The full system within the summation bound, the count exact; returns (terms, info) of the restatement."""
    info = {}
    terms = tc.spec_terms(rig.world, case, info)
    want, bound = tc.system_bound(terms)
    got = rig.system(case)
    assert got[28] == len(terms), f"{case}: {got[28]} pairs, spec {len(terms)}"
    assert len(terms) >= min_pairs, case
    bad = ~(np.abs(got - want) <= bound)
    assert not bad.any(), f"{case}: entries {np.nonzero(bad)[0].tolist()} differ: {got[bad]} vs {want[bad]} (bound {bound[bad]})"
    return terms, info


def check_single_pairs(rig, case, terms, info, picks):
    """Each picked pair alone: all 29 entries equal the double value of its float32 terms, count 1."""
    for idx in picks:
        got = rig.system(case.with_mask(tc.single_mask(case.hw, case.level, idx), f"pair {idx}"))
        want = terms[np.searchsorted(info["idx"], idx)].astype(np.float64)
        assert want[28] == 1.0
        assert np.all(got == want), f"{case} sample {idx}: entries {np.nonzero(got != want)[0].tolist()}: {got} vs {want}"
    return len(picks)


def spread(info, n):
    """n pairs spread over the pairs of a case."""
    idx = np.asarray(info["idx"])
    return [int(x) for x in idx[np.linspace(0, idx.size - 1, min(n, idx.size)).astype(int)]] if idx.size else []


def check_track(rig, case, vol=None):
    """Every result field of tsdf_track against the restatement's track; returns (pose entries that differ at all, worst
    difference in float32 ulps, the device's answer)."""
    hist = []
    want = tc.spec_track(rig.world, case, hist)
    assert tc.preconditions(hist, case.P()) == [], case
    got, st = rig.track(case, vol)
    assert (st["status"], st["iters_run"], st["inliers"]) == (want["status"], want["iters_run"], want["inliers"]), \
        f"{case}: {st} vs {want}"
    assert tc.ulps32(st["rmse"], want["rmse32"]) <= 1.0, f"{case}: rmse {st['rmse']!r} vs {want['rmse32']!r}"
    if want["lost"]:
        assert got.tobytes() == case.ref.tobytes(), f"{case}: a lost track returns the guess's own bits"
        return 0, 0.0, (got, st)
    u = tc.ulps32(got.ravel(), want["pose"])
    assert u.max() <= 1.0, f"{case}: pose entries {np.nonzero(u > 1.0)[0].tolist()} off by {u[u > 1.0]} float32 ulps"
    return int((u > 0).sum()), float(u.max()), (got, st)


def check_tracks(rig, cases, what):
    differ = worst = 0
    for c in cases:
        n, u, _ = check_track(rig, c)
        differ, worst = differ + n, max(worst, u)
    print(f"{what}: {len(cases)} tracks, {differ} pose entries differ from the restatement's at all (worst {worst:.2f} ulp)")


# ------------------------------------------------------------------------------------------------------------------------
def test_a_live_frame_value_edges(rig):
    singles = 0
    for c in tc.value_edge_cases(rig.world):
        terms, info = check_system(rig, c, min_pairs=50)
        singles += check_single_pairs(rig, c, terms, info, spread(info, 10))
    print(f"a: {singles} single-pair systems")


def test_b_relative_pose_edges(rig):
    singles = 0
    for c in tc.pose_edge_cases(rig.world):
        terms, info = check_system(rig, c)
        singles += check_single_pairs(rig, c, terms, info, tc.border_pairs(c.hw, info, cap=40))
    print(f"b: {singles} single-pair systems on the model's border")
    assert singles >= 200


def test_c_model_value_edges(rig):
    for c in tc.model_edge_cases(rig.world):
        terms, info = check_system(rig, c, min_pairs=50)
        check_single_pairs(rig, c, terms, info, spread(info, 5))


def test_d_tiny_images(rig):
    systems, tracks = tc.tiny_cases(rig.world)
    for c in systems:
        terms, info = check_system(rig, c)
        if ts.sample_grid(c.hw, c.level)[0].size == 0:
            assert len(terms) == 0 and not rig.system(c).any(), c                 # all zeros, count 0
        check_single_pairs(rig, c, terms, info, [int(x) for x in info["idx"]][:8])
    check_tracks(rig, tracks, "d")


@pytest.mark.parametrize("hw", tc.REDUCTION, ids=[f"{w}x{h}" for h, w in tc.REDUCTION])
def test_e_reduction_geometry(rig, hw):
    check_system(rig, tc.reduction_case(rig.world, hw), min_pairs=50)
    c = tc.reduction_case(rig.world, hw, close=True)
    terms, info = check_system(rig, c, min_pairs=50)
    picks = tc.nearest_pairs(info["idx"], tc.reduction_targets(hw))
    assert len(picks) >= 4, picks
    check_single_pairs(rig, c, terms, info, picks)
    mask, first = tc.last_workgroup_mask(hw)
    last = c.with_mask(mask, "last workgroup")
    _, li = check_system(rig, last, min_pairs=1)
    assert li["idx"].min() >= first


def test_f_state_machine(rig):
    check_tracks(rig, tc.state_machine_cases(rig.world), "f")


def test_g_handle_history(rig):
    calls = tc.history_calls(rig.world)

    def run(vol, c):
        if c.cur is None:
            pose, st = rig.track(c, vol)
            return pose.tobytes() + repr(sorted(st.items())).encode()
        return rig.system(c, vol).tobytes()

    with rig.fresh() as used:
        for k, c in enumerate(calls):
            got = run(used, c)
            with rig.fresh() as new:
                want = run(new, c)
            assert got == want, f"call {k} ({c}) on a used handle differs from a fresh one"
            if c.cur is None:
                check_track(rig, c, used)
            else:
                terms = tc.spec_terms(rig.world, c)
                want29, bound = tc.system_bound(terms)
                s = rig.system(c, used)
                assert s[28] == len(terms) and np.all(np.abs(s - want29) <= bound), c
