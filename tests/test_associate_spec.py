"""The association rule (csrc/tsdf_associate.hip.h and include/tsdf_hip.h, restated in tests/associate_spec.py) on hand-built
cases, without a GPU:

  * the per-pixel counts: live depth 0, NaN, +-inf, exactly near_m and far_m, exactly rdepth +- depth_tol_m and one float
    step beyond; pixels rendered with a non-finite render depth; member ids outside 0..M-1; overlapping masks; mask bytes
    around 128; members that are never rendered;
  * the assignment: IoU ties broken by k and then by m; one-to-one against best-per-mask where they differ; the label rule
    (same label, or a member score above 1.1 x the mask's); IoUs that only an exact comparison tells apart;
  * tsdf_associate_assign and tsdf_associate_params_default through ctypes (host only) against the spec on random count
    blocks, with counts near 2^31, and their refusals; the tsdf_associate_params / tsdf_associate_labels layouts.

The GPU tests (test_gpu_associate.py) hold the counting kernel and tsdf_batch_associate to the same spec."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import associate_spec as asp
from semantic_slam_amd import capi

f32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def block(agree, mask1, mem0, rng=None):
    """A consistent count block with the given overlap[k][m][agree], mask[k][1] and member[m][0]; the other words are 0 (or
    random below the ones the rule reads, with rng)."""
    agree = np.asarray(agree, np.uint64)
    K, M = agree.shape
    b = np.zeros(asp.n_words(K, M), np.uint64)
    ov, mk, mb = asp.split(b, K, M)
    ov[:, :, 0] = agree
    mk[:, 1] = mask1
    mb[:, 0] = mem0
    if rng is not None:
        ov[:, :, 1:] = rng.integers(0, 1000, (K, M, 2))
        mk[:, 0] = mk[:, 1] + rng.integers(0, 1000, K)
        mk[:, 2] = rng.integers(0, 1000, K)
        mb[:, 1:] = rng.integers(0, 1000, (M, 3))
    return b.astype(np.uint32)


def params(**kw):
    return asp.Params(**kw)


# ------------------------------------------------------------------------------------------------------------------------
# counts
# ------------------------------------------------------------------------------------------------------------------------
NEAR, FAR, TOL, RD = f32(0.5), f32(4.0), f32(0.0625), f32(2.0)


def edge_row():
    """One row of live depths against a render of member 0 at RD, with the class each pixel must get."""
    up = np.nextafter(RD + TOL, f32(np.inf))
    down = np.nextafter(RD - TOL, f32(-np.inf))
    cases = [(f32(0.0), 3), (f32(np.nan), 3), (f32(np.inf), 3), (f32(-np.inf), 3), (NEAR, 3),
             (np.nextafter(NEAR, f32(9)), 1), (FAR, 0 if abs(FAR - RD) <= TOL else 2), (np.nextafter(FAR, f32(9)), 3),
             (RD + TOL, 0), (RD - TOL, 0), (RD, 0), (up, 2), (down, 1), (f32(1.0), 1), (f32(3.0), 2)]
    return np.array([c[0] for c in cases], f32), np.array([c[1] for c in cases])


def test_live_depth_edges():
    d, want = edge_row()
    assert (d[8] - RD) == TOL and (RD - d[9]) == TOL             # the tolerance edges are exact in float32
    n = d.size
    member = np.zeros(n, np.int32)
    rd = np.full(n, RD, f32)
    p = params(near_m=NEAR, far_m=FAR, depth_tol_m=TOL)
    rendered, valid, cls = asp.classes(member, rd, d, 1, p)
    assert rendered.all()
    assert cls.tolist() == want.tolist()
    assert valid.tolist() == [c != 3 for c in want]
    masks = np.full((1, 1, n), 255, np.uint8)
    b = asp.counts(member.reshape(1, n), rd.reshape(1, n), d.reshape(1, n), masks, 1, p)
    ov, mk, mb = asp.split(b, 1, 1)
    assert mb[0].tolist() == [int((want == c).sum()) for c in range(4)]
    assert ov[0, 0].tolist() == mb[0, :3].tolist()
    assert mk[0].tolist() == [n, int((want != 3).sum()), 0]


def test_render_edges_and_unrendered_pixels():
    # member ids: -1 (miss), 0, 1, 2 (never rendered here), and ids no render writes (-5, 3, 99) count as not rendered
    member = np.array([[-1, 0, 1, -5, 3, 99, 0, 1]], np.int32)
    rd = np.array([[0.0, 1.0, np.nan, 1.0, 1.0, 1.0, np.inf, 1.0]], f32)
    d = np.array([[1.0, 1.0, 1.0, 1.0, 1.0, 0.0, 1.0, 0.0]], f32)
    p = params(near_m=0.1, far_m=6.0, depth_tol_m=0.01)
    masks = np.array([[[255, 255, 255, 255, 255, 255, 255, 255]]], np.uint8)
    b = asp.counts(member, rd, d, masks, 3, p)
    ov, mk, mb = asp.split(b, 1, 3)
    # member 0: pixel 1 agrees, pixel 6 (rdepth inf: r = -inf) is in front; member 1: pixel 2 (rdepth NaN) is behind,
    # pixel 7 live invalid
    assert mb.tolist() == [[1, 1, 0, 0], [0, 0, 1, 1], [0, 0, 0, 0]]
    assert ov[0].tolist() == [[1, 1, 0], [0, 0, 1], [0, 0, 0]]
    # in mask 8; live valid 6 (pixels 5 and 7 are 0); valid and not rendered: pixels 0, 3, 4
    assert mk[0].tolist() == [8, 6, 3]
    a, iou = asp.assign(b, 1, 3, params(min_pixels=1, min_iou=0.0))
    assert a.tolist() == [0]                               # member 2 has no pixel at all and is never a candidate


def test_overlapping_masks_and_mask_bytes():
    rng = np.random.default_rng(3)
    H, W, M = 9, 13, 4
    member = rng.integers(-1, M, (H, W)).astype(np.int32)
    rd = rng.uniform(1.0, 2.0, (H, W)).astype(f32)
    d = (rd + rng.choice([-0.1, 0.0, 0.1], (H, W))).astype(f32)
    base = rng.choice(np.array([0, 127, 128, 255], np.uint8), (H, W))
    masks = np.stack([base, base, np.where(base >= 128, 0, 200).astype(np.uint8)])   # 0 and 1 equal, 2 the complement
    p = params(depth_tol_m=0.05)
    ov, mk, mb = asp.split(asp.counts(member, rd, d, masks, M, p), 3, M)
    assert (ov[0] == ov[1]).all() and (mk[0] == mk[1]).all()
    assert (ov[0] + ov[2] == mb[:, :3]).all()              # a pixel is in mask 0 or in mask 2, and counted in each it is in
    assert mk[0, 0] + mk[2, 0] == H * W
    assert mk[0, 0] == int((base >= 128).sum())
    # and the per-pixel definition, directly
    s = base >= 128
    rendered = member >= 0
    valid = np.isfinite(d) & (d > p.near_m) & (d <= p.far_m)
    assert mk[0].tolist() == [s.sum(), (s & valid).sum(), (s & valid & ~rendered).sum()]
    for m in range(M):
        r = (d - rd).astype(f32)
        sel = s & (member == m) & valid
        assert ov[0, m].tolist() == [(sel & (np.abs(r) <= p.depth_tol_m)).sum(), (sel & (r < -p.depth_tol_m)).sum(),
                                     (sel & (np.abs(r) > p.depth_tol_m) & (r >= -p.depth_tol_m)).sum()]


# ------------------------------------------------------------------------------------------------------------------------
# assignment
# ------------------------------------------------------------------------------------------------------------------------
def test_iou_ties_break_by_k_then_m():
    p = params(min_pixels=1, min_iou=0.0)
    # every IoU 50 / 150: (0, 0) first, then (1, 1) -- (0, 1) and (1, 0) lose their mask or member
    b = block([[50, 50], [50, 50]], [100, 100], [100, 100])
    assert asp.assign(b, 2, 2, p)[0].tolist() == [0, 1]
    # one mask, three equal members: the lowest m; one member, two equal masks: the lowest k takes it
    assert asp.assign(block([[50, 50, 50]], [100], [100, 100, 100]), 1, 3, p)[0].tolist() == [0]
    assert asp.assign(block([[50], [50]], [100, 100], [100]), 2, 1, p)[0].tolist() == [0, -1]
    # equal fractions in different terms (50 / 150 and 100 / 300) are a tie too
    assert asp.assign(block([[50], [100]], [100, 300], [100]), 2, 1, p)[0].tolist() == [0, -1]
    # best per mask: ties to the lower m
    p0 = params(min_pixels=1, min_iou=0.0, one_to_one=0)
    assert asp.assign(block([[50, 50, 50]], [100], [100, 100, 100]), 1, 3, p0)[0].tolist() == [0]


def test_one_to_one_against_best_per_mask():
    b = block([[90, 80], [85, 0]], [100, 100], [100, 100])   # IoU (0,0) 90/110, (0,1) 80/120, (1,0) 85/115
    a1, i1 = asp.assign(b, 2, 2, params(min_pixels=1, min_iou=0.0, one_to_one=1))
    a0, i0 = asp.assign(b, 2, 2, params(min_pixels=1, min_iou=0.0, one_to_one=0))
    assert a1.tolist() == [0, -1] and a0.tolist() == [0, 0]
    assert i1[1] == 0.0 and i0[1] == f32(85 / 115) and i1[0] == i0[0] == f32(90 / 110)
    # and where greedy order matters: mask 1's best is member 0, which mask 0 takes first, so mask 1 falls back to member 1
    b = block([[90, 0], [85, 40]], [100, 100], [100, 100])
    assert asp.assign(b, 2, 2, params(min_pixels=1, min_iou=0.0))[0].tolist() == [0, 1]
    assert asp.assign(b, 2, 2, params(min_pixels=1, min_iou=0.0, one_to_one=0))[0].tolist() == [0, 0]


def test_thresholds():
    b = block([[25, 24]], [100], [25, 24])                 # IoU (0, 0) 25 / 100 exactly, (0, 1) 24 / 100
    assert asp.assign(b, 1, 2, params(min_pixels=25, min_iou=0.0))[0].tolist() == [0]
    assert asp.assign(b, 1, 2, params(min_pixels=26, min_iou=0.0))[0].tolist() == [-1]
    assert asp.assign(b, 1, 2, params(min_pixels=1, min_iou=0.25))[0].tolist() == [0]    # 25 >= 0.25 * 100
    assert asp.assign(b, 1, 2, params(min_pixels=1, min_iou=np.nextafter(f32(0.25), f32(1))))[0].tolist() == [-1]
    assert asp.assign(b, 1, 2, params(min_pixels=25, min_iou=0.24))[0].tolist() == [0]


def test_label_rule():
    b = block([[80]], [100], [100])
    p = params(min_pixels=1, min_iou=0.0)
    same = ([3], [0.9], [3], [0.5])                         # c3: the same label, whatever the scores
    veto = ([3], [0.9], [4], [0.9])                         # different labels, member score not above 1.1 x 0.9
    c4 = ([3], [0.9], [4], [1.0])                           # c4: 1.0 > 1.1f * 0.9f
    edge = ([3], [f32(0.5)], [4], [f32(1.1) * f32(0.5)])    # equal to 1.1f * score: not above
    assert asp.assign(b, 1, 1, p, same)[0].tolist() == [0]
    assert asp.assign(b, 1, 1, p, veto)[0].tolist() == [-1]
    assert asp.assign(b, 1, 1, p, c4)[0].tolist() == [0]
    assert asp.assign(b, 1, 1, p, edge)[0].tolist() == [-1]
    # the veto removes the candidate only: the mask then takes the next member that passes
    b = block([[80, 60]], [100], [100, 100])
    assert asp.assign(b, 1, 2, p, ([3], [0.9], [4, 3], [0.9, 0.1]))[0].tolist() == [1]


def exact_tie_breaker():
    """Two masks on one member whose IoUs agree as doubles but not exactly: 2^31 / (2^32 - 1) < (2^31 - 1) / (2^32 - 3)."""
    a = [[2 ** 31], [2 ** 31 - 1]]
    mask1 = [2 ** 32 - 1, 2 ** 32 - 4]
    mem0 = [2 ** 31]
    assert (2 ** 31) / (2 ** 32 - 1) == (2 ** 31 - 1) / (2 ** 32 - 3)      # doubles cannot tell them apart
    return block(a, mask1, mem0)


def test_iou_compared_exactly():
    a, iou = asp.assign(exact_tie_breaker(), 2, 1, params(min_pixels=1, min_iou=0.25))
    assert a.tolist() == [-1, 0]
    assert iou[1] == f32((2 ** 31 - 1) / (2 ** 32 - 3))


# ------------------------------------------------------------------------------------------------------------------------
# the library's host functions
# ------------------------------------------------------------------------------------------------------------------------
def lib_params(**kw):
    p = capi.associate_params_default(capi.default_config())
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def test_params_default():
    cfg = capi.make_config((64, 48, 32), 0.006, [0, 0, 0.5], max_depth=5.0)
    p = capi.associate_params_default(cfg)
    r = capi.raycast_params_default(cfg)
    assert bytes(p.ray) == bytes(r)
    assert p.depth_tol_m == f32(cfg.trunc_margin) == f32(0.006) * f32(5)
    assert (p.min_pixels, p.min_iou, p.one_to_one) == (25, f32(0.25), 1)


def test_library_assign_matches_the_spec_on_hand_cases():
    cases = [(block([[50, 50], [50, 50]], [100, 100], [100, 100]), 2, 2, dict(min_pixels=1, min_iou=0.0), None),
             (block([[90, 80], [85, 0]], [100, 100], [100, 100]), 2, 2, dict(min_pixels=1, min_iou=0.0, one_to_one=0), None),
             (block([[90, 0], [85, 40]], [100, 100], [100, 100]), 2, 2, dict(min_pixels=1, min_iou=0.0), None),
             (block([[80, 60]], [100], [100, 100]), 1, 2, dict(min_pixels=1, min_iou=0.0), ([3], [0.9], [4, 3], [0.9, 0.1])),
             (block([[80]], [100], [100]), 1, 1, dict(min_pixels=1, min_iou=0.0), ([3], [0.9], [4], [1.0])),
             (exact_tie_breaker(), 2, 1, dict(min_pixels=1), None)]
    for b, K, M, kw, lab in cases:
        want = asp.assign(b, K, M, params(**kw), lab)
        got = capi.associate_assign(lib_params(**kw), b, K, M, lab)
        assert got[0].tolist() == want[0].tolist() and got[1].tobytes() == want[1].tobytes(), (kw, got, want)
    assert capi.associate_assign(lib_params(min_pixels=1), exact_tie_breaker(), 2, 1)[0].tolist() == [-1, 0]


@pytest.mark.parametrize("scale", [100, 5000, 2 ** 31 - 2 ** 20], ids=["small", "image", "near2^31"])
def test_library_assign_matches_the_spec_on_random_blocks(scale):
    rng = np.random.default_rng(scale % 1000 + 7)
    for trial in range(60):
        K, M = int(rng.integers(1, 9)), int(rng.integers(1, 9))
        lo = scale // 2 if scale > 10 ** 6 else 0
        agree = rng.integers(lo, scale, (K, M), dtype=np.int64)
        agree = np.where(rng.random((K, M)) < 0.3, rng.integers(0, 30, (K, M)), agree)   # some below min_pixels
        if trial % 3 == 0:                                     # forced ties: repeated values
            agree = np.where(rng.random((K, M)) < 0.5, agree.flat[0], agree)
        mask1 = agree.max(axis=1) + rng.integers(0, max(2, scale // 4), K)
        mem0 = agree.max(axis=0) + rng.integers(0, max(2, scale // 4), M)
        mask1 = np.minimum(mask1, 2 ** 32 - 1)
        mem0 = np.minimum(mem0, 2 ** 32 - 1)
        b = block(agree, mask1, mem0, rng)
        kw = dict(min_pixels=int(rng.integers(1, 40)), min_iou=float(f32(rng.choice([0.0, 0.1, 0.25, 0.5]))),
                  one_to_one=int(trial % 2))
        lab = None
        if trial % 4 == 1:
            lab = (rng.integers(0, 3, K).astype(np.uint16), rng.uniform(0.5, 1, K).astype(f32),
                   rng.integers(0, 3, M).astype(np.uint16), rng.uniform(0.5, 1, M).astype(f32))
        want = asp.assign(b, K, M, params(**kw), lab)
        got = capi.associate_assign(lib_params(**kw), b, K, M, lab)
        assert got[0].tolist() == want[0].tolist(), (trial, kw)
        assert got[1].tobytes() == want[1].tobytes(), (trial, got[1], want[1])


def test_library_assign_refusals():
    lib = capi.load()
    b = block([[50]], [100], [100])
    out_a, out_i = np.zeros(1, np.int32), np.zeros(1, f32)

    def refused(p, what, counts=b, k=1, m=1, labels=None, a=out_a, i=out_i):
        rc = lib.tsdf_associate_assign(C.byref(p) if p is not None else None,
                                       counts.ctypes.data if counts is not None else None, k, m, labels,
                                       a.ctypes.data if a is not None else None, i.ctypes.data if i is not None else None)
        msg = lib.tsdf_last_error().decode()
        assert rc == -1 and what in msg, (rc, msg)

    refused(lib_params(), "NULL", counts=None)
    refused(lib_params(), "NULL", a=None)
    refused(lib_params(), "NULL", i=None)
    refused(None, "NULL parameters")
    refused(lib_params(), "k = 0", k=0)
    refused(lib_params(), "k = 257", k=257)
    refused(lib_params(), "n_members = 0", m=0)
    for field, value, what in (("depth_tol_m", 0.0, "depth_tol_m"), ("depth_tol_m", float("nan"), "depth_tol_m"),
                               ("depth_tol_m", float("inf"), "depth_tol_m"), ("min_pixels", 0, "min_pixels"),
                               ("min_iou", 1.5, "min_iou"), ("min_iou", -0.1, "min_iou"),
                               ("min_iou", float("nan"), "min_iou"), ("one_to_one", 2, "one_to_one")):
        refused(lib_params(**{field: value}), what)
    p = lib_params()
    p.ray.near_m = -1.0
    refused(p, "near")
    lab = capi.AssociateLabels(np.zeros(1, np.uint16).ctypes.data, None, None, None)
    refused(lib_params(), "label block", labels=C.byref(lab))
    refused(lib_params(min_pixels=1), "inconsistent", counts=block([[101]], [100], [200]))
    refused(lib_params(min_pixels=1), "inconsistent", counts=block([[101]], [200], [100]))
    a, i = capi.associate_assign(lib_params(min_pixels=1), b, 1, 1)       # and a good call still works
    assert a.tolist() == [0] and i[0] == f32(50 / 150)


def test_struct_layouts_match_c(tmp_path):
    prog = tmp_path / "layout.c"
    lines = ['printf("psize %zu\\n", sizeof(tsdf_associate_params));', 'printf("lsize %zu\\n", sizeof(tsdf_associate_labels));']
    lines += [f'printf("p.{f} %zu\\n", offsetof(tsdf_associate_params, {f}));' for f, _ in capi.AssociateParams._fields_]
    lines += [f'printf("l.{f} %zu\\n", offsetof(tsdf_associate_labels, {f}));' for f, _ in capi.AssociateLabels._fields_]
    prog.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "tsdf_hip.h"\nint main(void){\n' + "\n".join(lines) +
                    "\nreturn 0;}\n")
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(prog), "-o", str(exe)])
    got = dict(line.split() for line in subprocess.check_output([str(exe)]).decode().splitlines())
    assert int(got["psize"]) == C.sizeof(capi.AssociateParams)
    assert int(got["lsize"]) == C.sizeof(capi.AssociateLabels)
    for f, _ in capi.AssociateParams._fields_:
        assert int(got[f"p.{f}"]) == getattr(capi.AssociateParams, f).offset, f
    for f, _ in capi.AssociateLabels._fields_:
        assert int(got[f"l.{f}"]) == getattr(capi.AssociateLabels, f).offset, f
