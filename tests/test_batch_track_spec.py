"""Joint tracking against a batch (csrc/tsdf_batch_track.hip.h, restated in tests/batch_track_spec.py) means what it says, on
the CPU, with exact model maps of synth.ObjectScene (tests/batch_track_cases.py):

  * the restatement's one-pass split by member is the literal definition (track_spec.system on the render with depth 0
    everywhere but at member m) bit for bit, the used members' systems add up to the system on the masked model, and member
    ids no member has (-7, -1, M, M + 3) contribute to no member;
  * the joint system of the four objects is well conditioned, and a joint track recovers 1 deg / 1 cm guesses;
  * an object that was moved drags the joint pose away while every member's rmse looks alike; left out, the pose is right and
    that member's own rmse stands out;
  * every tracked case of tests/test_gpu_batch_track.py keeps clear of the restatement's thresholds on the exact model, from
    the guesses clear_seeds takes; the candidates passed over are the recorded ones;
  * the new calls are bound with their prototypes and refuse NULL arguments without a device."""
import ctypes as C

import numpy as np
import pytest

import batch_track_cases as bc
import batch_track_spec as bts
import track_cases as tc
import track_spec as ts
from semantic_slam_amd import capi, synth

f32 = np.float32
N = len(synth.OBJECTS)
SMALL = 2                        # 320 x 240 with the intrinsics halved: the size the conditioning figures were measured at


@pytest.fixture(scope="module")
def small():
    scene, true, live, moved = bc.frames(SMALL, wall=False)
    guess = bc.guess_of(true, 7)
    return scene, true, live, moved, guess, bc.exact_model(scene, guess)


# ------------------------------------------------------------------------------------------------------------------------
# the restatement against the rule's literal wording
# ------------------------------------------------------------------------------------------------------------------------
def test_member_split_is_the_literal_definition_and_adds_up(small):
    scene, true, live, _, guess, model = small
    P = bc.params(SMALL)
    M = ts.relative(guess, true)
    for level in range(3):
        sums, absums = bts.member_systems((live, None), model, N, level, M, P)
        for m in range(N):
            want, wabs = ts.system((live, None), bts.masked_model(*model, [m]), level, M, P)
            assert sums[m].tobytes() == want.tobytes() and absums[m].tobytes() == wabs.tobytes(), (level, m)
            assert sums[m, 28] > 100, (level, m, sums[m, 28])                      # no member is vacuous
        for use in (None, bc.all_but(1), [0, 1, 0, 1], [0, 0, 0, 0]):
            used = bts.used_members(N, use)
            terms, _ = ts.pair_terms((live, None), bts.masked_model(*model, used), level, M[:, :3].astype(f32),
                                     M[:, 3].astype(f32), P)
            want, bound = tc.system_bound(terms)
            got = sums[used].sum(axis=0) if used else np.zeros(29)
            assert got[28] == len(terms), (level, use)
            assert np.all(np.abs(got - want) <= bound), (level, use)


def test_ids_no_member_has_contribute_to_no_member(small):
    scene, true, live, _, guess, (depth, normal, ids) = small
    P = bc.params(SMALL)
    M = ts.relative(guess, true)
    rng = np.random.default_rng(3)
    member = ids.copy()
    on = np.flatnonzero(ids.ravel() >= 0)
    bad = rng.choice(on, on.size // 20, replace=False)
    member.ravel()[bad] = rng.choice(np.array([-7, -1, N, N + 3]), bad.size)
    info = {}
    ts.pair_terms((live, None), (depth, normal), 0, M[:, :3].astype(f32), M[:, 3].astype(f32), P, info)
    ui, vi = info["model_px"]
    landed = member[vi, ui]
    assert ((landed < 0) | (landed >= N)).sum() > 100                # pairs do land on the pixels that were given away
    sums, _ = bts.member_systems((live, None), (depth, normal, member), N, 0, M, P)
    for m in range(N):
        assert sums[m, 28] == (landed == m).sum(), m
    # and a member count below the ids in the image cuts the upper members off
    sums2, _ = bts.member_systems((live, None), (depth, normal, ids), 2, 0, M, P)
    full, _ = bts.member_systems((live, None), (depth, normal, ids), N, 0, M, P)
    assert sums2.shape == (2, 29) and sums2.tobytes() == full[:2].tobytes()


def test_result_pose_is_the_reference_camera_times_m(small):
    _, true, _, _, guess, _ = small
    M = ts.relative(guess, true)
    got = bts.result_pose(guess, M)
    # C_ref * (C_ref^T (C_cur - t_ref)): a float32 rotation is orthonormal to a few 2^-24 per entry, and the entries are <= 2
    assert np.abs(got.astype(np.float64) - true.astype(np.float64)).max() <= 16 * 2.0 ** -24
    eye = np.hstack([np.eye(3), np.zeros((3, 1))])
    assert bts.result_pose(guess, eye).tobytes() == np.asarray(guess, f32).tobytes()


# ------------------------------------------------------------------------------------------------------------------------
# what the feature is for
# ------------------------------------------------------------------------------------------------------------------------
def test_joint_system_is_well_conditioned_and_two_spheres_are_not(small):
    scene, true, live, _, _, _ = small
    P = bc.params(SMALL)
    model = bc.exact_model(scene, true)
    eye = ts.relative(true, true)
    sums, _ = bts.member_systems((live, None), model, N, 0, eye, P)

    def ratio(members):
        A, _, _, _ = ts.unpack(sums[members].sum(axis=0))
        w = np.linalg.eigvalsh(A)
        return w[0] / w[-1]

    joint, spheres = ratio([0, 1, 2, 3]), ratio([0, 2])
    print(f"smallest / largest eigenvalue of J^T J: all four objects {joint:.2e}, the two spheres alone {spheres:.2e}")
    assert joint > 1e-3                                              # measured 1.1e-2
    assert spheres < 1e-2 * joint                                    # rotation about the line through their centres is free


def test_joint_track_recovers_the_guess(small):
    scene, true, live, _, guess, model = small
    r = bts.track((live, None), model, N, None, bc.params(SMALL))
    e = ts.pose_error(bts.result_pose(guess, r["M"]), true)
    print(f"joint track, exact model, 320 x 240: {e[0]:.2e} m, {e[1]:.2e} rad; member rmse {bts.member_rmse(r['systems'])}")
    assert r["status"] == 0
    # the resolution of live normals taken over s pixels on curved surfaces, not the arithmetic: measured 7.9e-5 m, 6.1e-5 rad
    # from this guess and 1.6e-4 m, 0.8e-4 rad from another; the bounds are 2.5 x the worse of each
    assert e[0] < 4e-4 and e[1] < 2e-4, e


def test_a_moved_object_is_seen_once_it_is_left_out(small):
    scene, true, _, moved, guess, model = small
    P = bc.params(SMALL)
    r_all = bts.track((moved, None), model, N, None, P)
    r_out = bts.track((moved, None), model, N, bc.all_but(bc.MOVED), P)
    e_all = ts.pose_error(bts.result_pose(guess, r_all["M"]), true)
    e_out = ts.pose_error(bts.result_pose(guess, r_out["M"]), true)
    rm_all, rm_out = bts.member_rmse(r_all["systems"]), bts.member_rmse(r_out["systems"])
    print(f"moved box, all members: {e_all[0]:.2e} m, {e_all[1]:.2e} rad, member rmse {rm_all}")
    print(f"moved box, member {bc.MOVED} out: {e_out[0]:.2e} m, {e_out[1]:.2e} rad, member rmse {rm_out}")
    assert r_all["status"] != 2 and r_out["status"] != 2
    assert e_out[0] < e_all[0] and e_out[1] < e_all[1]
    assert int(np.argmax(rm_out)) == bc.MOVED
    assert (r_out["systems"][:, 28] > 100).all()                     # every member, used or not, has a system


def test_a_track_with_every_member_out_is_lost(small):
    _, _, live, _, guess, model = small
    r = bts.track((live, None), model, N, [0] * N, bc.params(SMALL))
    assert r["lost"] and r["status"] == 2 and r["inliers"] == 0
    assert not r["systems"].any() and r["systems"].shape == (N, 29)


# ------------------------------------------------------------------------------------------------------------------------
# the tracked cases of the GPU tests
# ------------------------------------------------------------------------------------------------------------------------
def test_tracked_gpu_cases_keep_clear_of_the_thresholds_on_the_exact_model():
    scene, true, live, moved = bc.frames(1)
    P = bc.params(1)

    def run(frame, uses):
        def breaches(guess):
            model = bc.exact_model(scene, guess)
            bad = []
            for use in uses:
                hist = []
                r = bts.track((frame, None), model, N, use, P, hist)
                assert not r["lost"]
                bad += tc.preconditions(hist, P)
            return bad
        return breaches

    taken, passed = bc.clear_seeds(true, run(live, [None]), bc.N_PRODUCT_GUESSES)
    print("product:", taken, passed)
    assert [s for s, _ in passed] == bc.PASSED_OVER_EXACT["product"]
    taken, passed = bc.clear_seeds(true, run(moved, [None, bc.all_but(bc.MOVED)]), 1)
    print("moved:", taken, passed)
    assert [s for s, _ in passed] == bc.PASSED_OVER_EXACT["moved"]


# ------------------------------------------------------------------------------------------------------------------------
# the binding, without a device
# ------------------------------------------------------------------------------------------------------------------------
def test_calls_are_bound_and_refuse_null_without_a_device():
    lib = capi.load()
    for name in ("tsdf_batch_track", "tsdf_batch_track_system", "tsdf_track_member_systems"):
        assert name in capi.ABI_SYMBOLS and getattr(lib, name).argtypes, name
    assert len(lib.tsdf_batch_track.argtypes) == 8 and len(lib.tsdf_track_member_systems.argtypes) == 12
    cfg = capi.default_config(480, 640)
    p = capi.track_params_default(cfg)
    assert (p.n_levels, list(p.iters), p.min_inliers) == (3, [10, 5, 4], 300)       # the defaults the batch calls take
    out, eye, res = np.zeros((2, 29)), np.eye(4, dtype=f32).ravel(), capi.TrackResult()
    buf = np.zeros(16, f32)
    rc = lib.tsdf_batch_track(None, C.byref(p), buf.ctypes.data, None, None, eye.ctypes.data, C.byref(res), None)
    assert rc == -1 and "tsdf_batch_track: NULL" in lib.tsdf_last_error().decode()
    rc = lib.tsdf_batch_track_system(None, C.byref(p), buf.ctypes.data, None, eye.ctypes.data, eye.ctypes.data, 0,
                                     out.ctypes.data)
    assert rc == -1 and "tsdf_batch_track_system: NULL" in lib.tsdf_last_error().decode()
    rc = lib.tsdf_track_member_systems(0, C.byref(p), None, None, None, 2, None, None, eye.ctypes.data, eye.ctypes.data, 0,
                                       out.ctypes.data)
    assert rc == -1 and "tsdf_track_member_systems: NULL" in lib.tsdf_last_error().decode()
    for n in (0, 65537):                                             # the sizes are refused before any device is touched
        rc = lib.tsdf_track_member_systems(0, C.byref(p), 8, 8, 8, n, 8, None, eye.ctypes.data, eye.ctypes.data, 0,
                                           out.ctypes.data)
        assert rc == -1 and f"n_members = {n}" in lib.tsdf_last_error().decode()
    rc = lib.tsdf_track_member_systems(0, C.byref(p), 8, 8, 8, 2, 8, None, eye.ctypes.data, eye.ctypes.data, 3, out.ctypes.data)
    assert rc == -1 and "level 3" in lib.tsdf_last_error().decode()
    for name in ("track", "track_system"):
        assert callable(getattr(capi.Batch, name))
    assert callable(capi.track_member_systems)
