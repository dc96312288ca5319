"""The carry rule (csrc/tsdf_fuse_carry.hip.h) in its NumPy restatement tests/fuse_carry_spec.py, without a GPU: the C
struct and flags, the identities the rule was built to have (carry 0 is the merge; a lattice shift copies bits; half-voxel
ties go to the upper corner and round away from zero; one frame's votes are folded in as that frame would have been), the
clamp branches, and that no case of tests/test_gpu_fuse_carry.py is vacuous."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import fuse_carry_cases as cc
import fuse_carry_spec as fcs
import fuse_spec as fs
from semantic_slam_amd import capi, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
ALL_CASES = [(d, p, s) for d in cc.DST_SHAPES for p in range(cc.N_POSES) for s in cc.STATES]


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def test_struct_layout_flags_and_host_refusals(tmp_path):
    fields = [f for f, _ in capi.FuseCarryCounts._fields_]
    body = 'printf("size %zu\\n", sizeof(tsdf_fuse_carry_counts));\n'
    body += "".join(f'printf("{f} %zu\\n", offsetof(tsdf_fuse_carry_counts, {f}));\n' for f in fields)
    body += 'printf("colour %u\\nlabels %u\\n", TSDF_FUSE_CARRY_COLOUR, TSDF_FUSE_CARRY_LABELS);\n'
    prog = tmp_path / "layout.c"
    prog.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "tsdf_hip.h"\nint main(void){\n' + body + "return 0;}\n")
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(prog), "-o", str(exe)])
    got = dict(line.split() for line in subprocess.check_output([str(exe)]).decode().splitlines())
    assert int(got["size"]) == C.sizeof(capi.FuseCarryCounts)
    for f in fields:
        assert int(got[f]) == getattr(capi.FuseCarryCounts, f).offset, f
    assert (int(got["colour"]), int(got["labels"])) == (capi.FUSE_CARRY_COLOUR, capi.FUSE_CARRY_LABELS) == (fcs.COLOUR, fcs.LABELS)
    assert fields == list(fcs.CARRY_COUNT_NAMES)
    lib = capi.load()
    p = capi.fuse_params_default(capi.default_config())
    assert lib.tsdf_fuse_volume_carry(None, None, C.byref(p), None, 3, None, None) == -1
    assert b"tsdf_fuse_volume_carry" in lib.tsdf_last_error() and b"NULL" in lib.tsdf_last_error()
    assert lib.tsdf_upload_labels(None, None, None, None) == -1 and b"tsdf_upload_labels" in lib.tsdf_last_error()
    assert lib.tsdf_upload_colour(None, None) == -1 and b"tsdf_upload_colour" in lib.tsdf_last_error()


def test_the_gpu_parity_cases_are_not_vacuous():
    """Every "edges" case carries at least a tenth of the destination and meets both branches of the colour blend and all
    four of the label rule; every "surf" case adopts, agrees and opposes, and together they flip and keep.  The shapes are
    16-byte rows with last x tiles of 8, 3 and 1 quads and z extents that are no multiple of a workgroup's 16 slices."""
    surf_flipped = surf_kept = 0
    for dims, pose, state in ALL_CASES:
        *_, counts, info = cc.parity_case(dims, pose, state, 3)
        what = (dims, pose, state, {k: info[k] for k in ("carried", "fresh", "blended", "adopted", "agreed", "flipped", "opposed_kept")})
        assert info["carried"] == counts["sampled"], what
        assert counts["label_opposed"] == info["flipped"] + info["opposed_kept"] and counts["label_flipped"] == info["flipped"]
        if state == "edges":
            assert info["carried"] >= 0.10 * np.prod(dims), what
            assert min(info[k] for k in ("fresh", "blended", "adopted", "agreed", "flipped", "opposed_kept")) > 0, what
            assert info["at_threshold"] > 0, what                      # equal evidence: the voxel keeps its label
            assert all(0.3 * info["carried"] < u < 0.7 * info["carried"] for u in info["upper"]), what
        else:
            assert min(info[k] for k in ("adopted", "agreed")) > 0 and counts["label_opposed"] > 0, what
            surf_flipped += info["flipped"]
            surf_kept += info["opposed_kept"]
    assert surf_flipped > 0 and surf_kept > 0
    assert all(d[0] % 4 == 0 for d in cc.DST_SHAPES)
    assert sorted(((d[0] // 4 - 1) % 8) + 1 for d in cc.DST_SHAPES) == [1, 3, 8]
    assert all(d[0] > 32 or d[1] > 8 or d[2] > 16 for d in cc.DST_SHAPES) and all(d[2] % 16 for d in cc.DST_SHAPES)


@pytest.mark.parametrize("dims,pose,state", ALL_CASES[::3])
def test_carry_zero_is_the_merge(dims, pose, state):
    dcfg, scfg, dst, src = cc.states(dims, pose, state)
    for write in (0, 1):
        want_t, want_w, want_counts = fs.fuse(dst[0], dst[1], fs.grid_of(dcfg), src[0], src[1], fs.grid_of(scfg),
                                              weight_thresh=0.9, agree_tol=0.4, write=write)
        got, counts = fcs.fuse_carry(dst, fs.grid_of(dcfg), src, fs.grid_of(scfg), 0, write=write)
        assert np.array_equal(bits(got[0]), bits(want_t)) and np.array_equal(bits(got[1]), bits(want_w))
        assert counts == dict(want_counts, **dict.fromkeys(fcs.CARRY_COUNT_NAMES, 0))
        for a, b in zip(got[2:], dst[2:]):
            assert np.array_equal(bits(a), bits(b))
        for carry in (1, 2, 3):                                        # the geometry never depends on what is carried
            more, more_counts = fcs.fuse_carry(dst, fs.grid_of(dcfg), src, fs.grid_of(scfg), carry, write=write)
            assert np.array_equal(bits(more[0]), bits(want_t)) and np.array_equal(bits(more[1]), bits(want_w))
            assert {k: more_counts[k] for k in fs.COUNT_NAMES} == want_counts
            if not carry & fcs.COLOUR or not write:
                assert np.array_equal(more[2], dst[2])
            if not carry & fcs.LABELS or not write:
                assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(more[3:], dst[3:]))
            if not carry & fcs.LABELS:
                assert all(more_counts[k] == 0 for k in fcs.CARRY_COUNT_NAMES)
        if write == 0:
            dry = more_counts
    assert dry == more_counts                                          # carry 3: the eight counts do not depend on write


def test_lattice_shift_copies_attribute_bits():
    dg, sg, dst, src, want, taken = cc.lattice_copy_case()
    info = {}
    got, counts = fcs.fuse_carry(dst, dg, src, sg, 3, info=info)
    assert not info["f"].any() and info["carried"] == taken == counts["sampled"] and info["fresh"] == taken
    for name, a, b in zip(("tsdf", "weight", "colour", "label", "fp", "bp"), got, want):
        assert np.array_equal(bits(a), bits(b)), name
    labelled = int((want[3] != 0).sum())
    assert 0 < labelled < taken
    assert counts["label_adopted"] == labelled and counts["label_agreed"] == counts["label_opposed"] == 0


def test_half_voxel_ties_take_the_upper_corner_and_round_away_from_zero():
    dg, sg, dst, src = cc.half_voxel_case()
    info = {}
    got, counts = fcs.fuse_carry(dst, dg, src, sg, 3, info=info)
    (sx, sy, sz), (dx, dy, dz) = sg[0], dg[0]
    assert info["carried"] == (sx - 1) * (sy - 1) * (sz - 1) == info["ties"] and np.all(info["f"] == f32(0.5))
    assert info["upper"] == [info["carried"]] * 3
    # destination voxel (x, y, z) sits at source position (x - 8.5, y - 4.5, z - 0.5): its cell spans x - 9 .. x - 8, ...
    col, lab, fp, bp = (a.reshape(sz, sy, sx) for a in src[2:])
    box = (slice(1, sz), slice(5, 4 + sy), slice(9, 8 + sx))
    want_lab = np.zeros((dz, dy, dx), np.uint16)
    want_lab[box] = lab[1:, 1:, 1:]                                     # the upper corner on every axis
    assert np.array_equal(got[3], want_lab.ravel())
    for got_a, a in ((got[4], fp), (got[5], bp)):
        full = np.zeros((dz, dy, dx), f32)
        full[box] = a[1:, 1:, 1:]
        assert np.array_equal(bits(got_a), bits(full.ravel()))
    # colour: the mean of the cell's eight corners is exact in float32 (eighths), and a half rounds up; the red channel depends
    # on x alone, so its mean is that of two values
    kinds = {}
    for shift, name in ((0, "two"), (8, "eight")):
        c = ((col >> np.uint32(shift)) & np.uint32(255)).astype(np.int64)
        total = sum(c[a:sz - 1 + a, b:sy - 1 + b, d:sx - 1 + d] for a in (0, 1) for b in (0, 1) for d in (0, 1))
        want_c = (total + 4) // 8                                       # floor(total / 8 + 1 / 2)
        got_c = ((got[2].reshape(dz, dy, dx)[box] >> np.uint32(shift)) & np.uint32(255)).astype(np.int64)
        assert np.array_equal(got_c, want_c), name
        kinds[name] = int((total % 8 == 4).sum())
        if name == "two":
            pair = c[0, 0, :-1] + c[0, 0, 1:]
            assert np.array_equal(total, np.broadcast_to(4 * pair, total.shape))
            assert np.array_equal(want_c, np.broadcast_to((pair + 1) // 2, want_c.shape))
    assert kinds["two"] > 0 and kinds["eight"] > 0, kinds
    assert info["half_up"] >= kinds["two"] + kinds["eight"]
    assert np.all(got[2].reshape(dz, dy, dx)[0] == 0) and np.all(got[2] >> np.uint32(24) == 0)


def test_one_frames_votes_are_folded_in_as_that_frame(oracle):
    """A destination with two frames of label evidence; a source on the same grid that holds exactly one further frame.  The
    carried labels, Fp and Bp equal Oracle.integrate_labels of that frame on the destination, in every voxel."""
    dims, vs = (48, 48, 48), 2.0 ** -6
    origin = np.array([-24 * vs, -24 * vs, 52 * vs], f32)
    h, w = 120, 160
    K = synth.TUM_K.copy()
    K[[0, 2, 4, 5]] *= 0.25
    eye = np.eye(4, dtype=f32).ravel()
    scene = synth.SurfScene(dims, vs, origin, K=K, h=h, w=w)
    trunc = float(f32(vs) * f32(5))
    grid = (dims, origin, vs, trunc)
    n = int(np.prod(dims))
    rng = np.random.default_rng(4)
    label_ims = [np.repeat(np.repeat(rng.integers(0, 4, (h // 8, w // 8)).astype(np.uint16), 8, 0), 8, 1) for _ in range(3)]
    score_ims = [rng.uniform(0.3, 0.99, (h, w)).astype(f32) for _ in range(3)]
    dt, dw = oracle.init_grid(dims)
    dlab, dfp, dbp = np.zeros(n, np.uint16), np.zeros(n, f32), np.zeros(n, f32)
    poses = [scene.pose(k, n=8) for k in range(3)]
    frames = [(oracle.cam2base(eye, c2w), scene.depth(c2w, quantize=True)) for c2w in poses]
    for k in range(2):
        oracle.integrate(K, frames[k][0], frames[k][1], *grid, dt, dw)
        oracle.integrate_labels(K, frames[k][0], frames[k][1], label_ims[k], score_ims[k], *grid, dlab, dfp, dbp, prob_thd=0.5)
    st, sw = oracle.init_grid(dims)
    slab, sfp, sbp = np.zeros(n, np.uint16), np.zeros(n, f32), np.zeros(n, f32)
    oracle.integrate(K, frames[2][0], frames[2][1], *grid, st, sw)
    oracle.integrate_labels(K, frames[2][0], frames[2][1], label_ims[2], score_ims[2], *grid, slab, sfp, sbp, prob_thd=0.5)
    want = dlab.copy(), dfp.copy(), dbp.copy()
    oracle.integrate_labels(K, frames[2][0], frames[2][1], label_ims[2], score_ims[2], *grid, *want, prob_thd=0.5)
    g = (dims, origin, f32(vs), f32(trunc), eye)
    zeros = np.zeros(n, np.uint32)
    info = {}
    got, counts = fcs.fuse_carry((dt, dw, zeros, dlab, dfp, dbp), g, (st, sw, zeros, slab, sfp, sbp), g, 2, prob_thd=0.5, info=info)
    assert not info["f"].any()
    assert np.all(info["valid"][slab != 0]), "every voxel the frame voted on is carried"
    assert min(counts[k] for k in fcs.CARRY_COUNT_NAMES) > 0 and info["opposed_kept"] > 0, counts
    for name, a, b in zip(("label", "fp", "bp"), got[3:], want):
        assert np.array_equal(bits(a), bits(b)), name
    assert (got[3] != dlab).sum() >= counts["label_adopted"] > 0


def test_every_clamp_branch_is_reached_in_the_edge_cases():
    """r > 255, r < 0 and a NaN: reached through destination weights that are NaN, negative or that cancel the sample's."""
    for dims, pose, state in ALL_CASES:
        *_, want, counts, info = cc.parity_case(dims, pose, state, 3)
        if state == "edges":
            assert info["clamp_hi"] > 0 and info["clamp_neg"] > 0 and info["clamp_nan"] > 0, (dims, pose, info)
        else:
            assert info["clamp_hi"] == info["clamp_neg"] == info["clamp_nan"] == 0
        assert np.all(want[2] >> np.uint32(24) == 0)
