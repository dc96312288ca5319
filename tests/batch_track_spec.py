"""Float32 NumPy restatement of joint tracking against a batch (csrc/tsdf_batch_track.hip.h states the rule), a thin layer over
tests/track_spec.py, which restates tsdf_track's rule and stays as it is.  The rule is tsdf_track's with three changes:

  Frame    the poses are taken in the reference camera's frame: C_ref is the float32 ref_cam2world itself, C_cur the float32
           cam2world (no base2world enters: the members have base frames of their own); M = track_spec.relative(C_ref, C_cur);
           the result is cam2world = C_ref * M in double, rounded to float32: track_spec.result_pose with an identity base.
  Model    the batch's render at C_ref: depth, normal and member index per pixel.  A pair is rejected at the model-pixel gate
           unless t > 0, nm != 0 and 0 <= member[pixel] < n_members, for the joint system also unless use[member[pixel]] != 0;
           it belongs to the member of its model pixel.
  Systems  S[m] is the sum of the 29 float32 terms over member m's pairs; the joint system of an iteration is the sum over
           the pairs of the used members, and everything else (solve, lost test, step, levels, status, iters_run, inliers,
           rmse) is track_spec.track's on it.  After the last iteration one more pass evaluates S[m] for every member, used or
           not, at the final estimate and at the finest level with iters > 0 (level 0 when none has); on a lost track every
           S[m] is zero and the pose is the guess's own bits.  The counts S[m][28] are of that later pass, not of the
           iteration `inliers` reports.

Consequence (what this module is built on): the joint track is track_spec.track on the render with depth 0 wherever the member
is outside [0, n_members) or is not used; S[m] is track_spec.system on the render with depth 0 everywhere but at member m.
Zeroing the depth of a model pixel rejects exactly the pairs that land on it (t > 0 fails) and changes no other pair, so one
pass over the render with the out-of-range members zeroed, split by the member of each pair's model pixel, gives the same
per-member terms bit for bit; member_terms does that (M times cheaper), and tests/test_batch_track_spec.py checks it against
the literal definition.

    masked_model(depth, normal, member, keep)              (depth', normal): depth 0 where member is not in keep
    member_terms(live, model, n_members, level, M, P)      (terms [n, 29] float32, owner [n]: the member of each pair, info)
    member_systems(live, model, n_members, level, M, P)    (sums [n_members, 29] float64, sums of |term| [n_members, 29])
    track(live, model, n_members, use, P, history=None)    track_spec.track's dict and "level", "systems", "abs_systems",
                                                           "counts" (terms per member of the final pass, for the bound)
    result_pose(c_ref, M)                                  cam2world float32 [16]

live = (depth [H, W], mask or None); model = (depth [H, W], normal [H, W, 3], member [H, W] int32); use: None (all) or one flag
per member; P: a track_spec params dict."""
import numpy as np

import track_spec as ts

f32 = np.float32
N_TERMS = ts.N_TERMS


def masked_model(depth, normal, member, keep):
    """keep: the member ids whose pixels stay (any iterable of ints; ids no member has are simply not there)."""
    keep = np.asarray(sorted(set(int(k) for k in keep)), np.int64)
    on = np.isin(np.asarray(member), keep)
    return np.where(on, np.asarray(depth, f32), f32(0)), np.asarray(normal, f32)


def used_members(n_members, use):
    return list(range(n_members)) if use is None else [m for m in range(n_members) if use[m]]


def member_terms(live, model, n_members, level, M, P, info=None):
    depth, normal, member = model
    info = {} if info is None else info
    M = np.asarray(M, np.float64)
    terms, _ = ts.pair_terms(live, masked_model(depth, normal, member, range(n_members)), level, M[:, :3].astype(f32),
                             M[:, 3].astype(f32), P, info)
    ui, vi = info["model_px"]
    owner = np.asarray(member)[vi, ui].astype(np.int64)
    assert owner.size == 0 or (owner.min() >= 0 and owner.max() < n_members)
    return terms, owner, info


def member_systems(live, model, n_members, level, M, P):
    terms, owner, _ = member_terms(live, model, n_members, level, M, P)
    t64 = terms.astype(np.float64)
    sums, absums = np.zeros((n_members, N_TERMS)), np.zeros((n_members, N_TERMS))
    for m in np.unique(owner):
        sel = t64[owner == m]
        sums[m], absums[m] = sel.sum(axis=0), np.abs(sel).sum(axis=0)
    return sums, absums


def result_pose(c_ref, M):
    return ts.result_pose(np.eye(4, dtype=f32), c_ref, M)


def final_level(P):
    ran = [lvl for lvl in range(P["n_levels"]) if P["iters"][lvl] > 0]
    return ran[0] if ran else 0


def track(live, model, n_members, use, P, history=None):
    depth, normal, member = model
    r = ts.track(live, masked_model(depth, normal, member, used_members(n_members, use)), P, history=history)
    r["level"] = final_level(P)
    if r["lost"]:
        r["systems"] = np.zeros((n_members, N_TERMS))
        r["abs_systems"] = np.zeros((n_members, N_TERMS))
        r["counts"] = np.zeros(n_members, np.int64)
    else:
        r["systems"], r["abs_systems"] = member_systems(live, model, n_members, r["level"], r["M"], P)
        r["counts"] = r["systems"][:, 28].astype(np.int64)
    return r


def member_rmse(systems):
    """sqrt(S[27] / S[28]) per member (0 where a member has no pair)."""
    s = np.asarray(systems, np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(s[:, 28] > 0, np.sqrt(s[:, 27] / s[:, 28]), 0.0)
