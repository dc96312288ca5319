"""The cases of tests/test_gpu_batch_track.py (test infrastructure), shared with tests/test_batch_track_spec.py, which checks on
the CPU that every tracked case keeps clear of the restatement's own decision thresholds and that the behaviour the feature
exists for holds for the restatement: a joint track over synth.ObjectScene's four objects is well conditioned, and an object
that was moved drags the joint pose away while every member's rmse still looks alike, until it is left out.

The model of the CPU tests is exact: ObjectScene's depth, analytic normals and object ids at the guess.  The GPU tests feed
the restatement the device's own batch render.  Which guess keeps a track clear of the thresholds depends on the model, so
both take their guesses through clear_seeds: the candidate seeds in order, passing over those whose restatement run comes
within the margins of track_cases.preconditions (the choice never looks at the code under test).  The candidates the exact
model passes over are recorded in PASSED_OVER_EXACT; the GPU tests print theirs."""
import math

import numpy as np

import track_spec as ts
from semantic_slam_amd import synth

f32 = np.float32
POSE = 5                                      # of ObjectScene's 16-pose orbit; the members are fused from 0, 2, .., 14
COS_WIDE = math.cos(math.radians(40.0))
MIN_INLIERS = 100
MOVED, SHIFT_M = 1, 0.03                      # box 1 sits 3 cm nearer to the camera in the moved-object frame
CANDIDATE_SEEDS = tuple(range(7, 15))         # of the 1 deg / 1 cm guesses, tried in this order (clear_seeds)
N_PRODUCT_GUESSES = 2
# the candidates the exact-model runs of tests/test_batch_track_spec.py pass over at 640 x 480, each for one step with
# |w| / eps_rot inside [0.9, 1.1]: the product case takes seeds 8 and 9, the moved-object frame seed 9
PASSED_OVER_EXACT = {"product": [7], "moved": [7, 8]}
FAR_WALL = 100.0                              # "no wall": beyond far_m, so its pixels are not valid depths


def scaled_K(scale):
    K = synth.TUM_K.astype(np.float64).copy()
    K[[0, 2, 4, 5]] /= scale
    return K.astype(f32)


def scene_of(scale=1, objects=synth.OBJECTS, wall=True):
    return synth.ObjectScene(objects, wall_z=2.0 if wall else FAR_WALL, K=scaled_K(scale), h=480 // scale, w=640 // scale)


def moved_objects(pose):
    """OBJECTS with box MOVED shifted SHIFT_M toward the camera of `pose` (along its optical axis; the box stays axis-aligned
    in the base frame)."""
    T = np.asarray(pose, np.float64).reshape(4, 4)
    shift = -SHIFT_M * T[:3, 2]
    objs = list(synth.OBJECTS)
    kind, lo, hi = objs[MOVED]
    assert kind == "box"
    objs[MOVED] = (kind, tuple(np.asarray(lo) + shift), tuple(np.asarray(hi) + shift))
    return tuple(objs)


def object_normals(scene, pose):
    """Analytic camera-frame normals of an ObjectScene at pose, toward the camera; (0, 0, 0) off the objects."""
    T = np.asarray(pose, np.float64).reshape(4, 4)
    z, who = scene._hit(T)
    z = np.where(np.isfinite(z), z, 0.0)
    P = T[:3, 3] + z[..., None] * (scene.dir_cam @ T[:3, :3].T)
    n = np.zeros(P.shape)
    for i, (kind, a, b) in enumerate(scene.objects):
        on = who == i
        if kind == "sphere":
            n[on] = (P[on] - a) / b
        else:
            d = np.concatenate([np.abs(P[on] - a), np.abs(P[on] - b)], axis=1)       # distance to the six faces
            face = d.argmin(axis=1)
            out = np.zeros((face.size, 3))
            out[np.arange(face.size), face % 3] = np.where(face < 3, -1.0, 1.0)
            n[on] = out
    return (n @ T[:3, :3]).astype(f32)                                               # R^T n


def exact_model(scene, pose):
    """(depth, normal, member) of the scene's objects at pose: what a perfect batch of one member per object renders."""
    ids = scene.ids(pose)
    return np.where(ids >= 0, scene.depth(pose), f32(0)).astype(f32), object_normals(scene, pose), ids


def params(scale=1, **kw):
    kw.setdefault("cos_thresh", COS_WIDE)
    kw.setdefault("min_inliers", MIN_INLIERS)
    return ts.params(scaled_K(scale), (480 // scale, 640 // scale), **kw)


def guess_of(true, seed):
    return ts.perturb(true, np.random.default_rng(seed), 1.0, 0.01)


def clear_seeds(true, breaches, want, seeds=CANDIDATE_SEEDS):
    """The first `want` of the candidate seeds whose guess keeps every run that uses it clear of the restatement's thresholds:
    breaches(guess) runs the restatement (never the code under test) and returns track_cases.preconditions' list, over
    every call made from that guess.  Returns (seeds taken, [(seed passed over, its breaches)])."""
    taken, passed = [], []
    for s in seeds:
        bad = breaches(guess_of(true, s))
        if bad:
            passed.append((s, bad))
            continue
        taken.append(s)
        if len(taken) == want:
            return taken, passed
    raise AssertionError(f"only {taken} of {seeds} keep clear of the thresholds: {passed}")


def frames(scale=1, wall=True):
    """(scene, true pose, live frame, live frame with box MOVED shifted) of the tracked cases."""
    scene = scene_of(scale, wall=wall)
    true = scene.pose(POSE)
    return scene, true, scene.depth(true), scene_of(scale, moved_objects(true), wall=wall).depth(true)


def all_but(m, n=len(synth.OBJECTS)):
    return [int(k != m) for k in range(n)]
