"""The extent of fused volumes on the device (csrc/tsdf_extent.hip.h: tsdf_volume_extent, tsdf_batch_extents,
tsdf_group_extent) against its integer restatement (tests/extent_spec.py), every field equal: aligned and unaligned rows,
partial workgroups, random, edge-valued and fused states, margins and bands; z-slabs and a group against the whole grid;
a batch with collected frames in one launch; that the call only reads; an outgrown object moved into the proposed grid;
and the refusals of the C ABI."""
import ctypes as C

import numpy as np
import pytest

import extent_cases as ec
import extent_spec as es
import fuse_cases as fc
from semantic_slam_amd import capi, synth

pytestmark = pytest.mark.gpu

f32 = np.float32


def bits_equal(a, b):
    return np.array_equal(np.asarray(a, f32).view(np.uint32), np.asarray(b, f32).view(np.uint32))


def integrate_fused(cuda, vol, dims):
    """The four frames of the case's fused state as one fused sequence (the summary words end up as a real run leaves them)."""
    poses, depths = ec.frames(dims)
    dev = [cuda.from_numpy(d).cuda() for d in depths]
    vol.integrate_frames_device([d.data_ptr() for d in dev], poses)
    vol.sync()


# ------------------------------------------------------------------------------------------------------------------------
# parity with the restatement
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims,state", [(d, s) for s in ec.STATES for d in ec.SHAPES if s in ec.states_of(d)],
                         ids=lambda v: v if isinstance(v, str) else "x".join(map(str, v)))
def test_parity_with_the_restatement(cuda, dims, state):
    n = int(np.prod(dims))
    with capi.Volume(ec.config(dims)) as vol:
        if state == "fused":
            integrate_fused(cuda, vol, dims)
        else:
            vol.upload(*ec.state(dims, state))
        t, w = vol.download()
        for band in ec.BANDS:
            for margin in ec.margins(dims):
                got = vol.extent(ec.params(band, margin)).as_dict()
                want = es.extent(t, w, dims, weight_thresh=ec.WEIGHT_THRESH, band=band, margin=margin)
                print(f"{dims} {state} band {band} margin {margin}: device {got}")
                assert got == want, (band, margin, want)
                assert want["n_surface"] >= 0.10 * n and want["n_observed"] - want["n_surface"] >= 0.01 * n
        t1, w1 = vol.download()
    assert bits_equal(t, t1) and bits_equal(w, w1)


# ------------------------------------------------------------------------------------------------------------------------
# slabs and a group
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("state", ["random", "edges"])
def test_slab_records_combine_to_the_whole_grids(cuda, state):
    dims = (20, 12, 9)
    t, w = ec.state(dims, state)
    slice_n = dims[0] * dims[1]
    p = ec.params(1.0, 1)
    with capi.Volume(ec.config(dims)) as whole:
        whole.upload(t, w)
        want = whole.extent(p).as_dict()
    assert want == es.extent(t, w, dims, margin=1)
    acc = None
    for a, b in ((0, 3), (3, 7), (7, 9)):
        with capi.Volume(ec.config(dims, z_begin=a, z_end=b)) as slab:
            slab.upload(t[a * slice_n:b * slice_n], w[a * slice_n:b * slice_n])
            rec = slab.extent(p)
        part = es.extent(t[a * slice_n:b * slice_n], w[a * slice_n:b * slice_n], dims, a, b, margin=1)
        print(f"slab [{a},{b}): {rec.as_dict()}")
        assert rec.as_dict() == part
        assert a <= part["lo"][2] <= part["hi"][2] < b                # z bounds are global
        assert (a == 0 or part["border"][4] == 0) and (b == dims[2] or part["border"][5] == 0)   # and so are the z faces
        acc = rec if acc is None else capi.extent_combine(acc, rec)
    assert acc.as_dict() == want


def test_group_of_three_slabs_equals_the_whole_grid_handle(cuda):
    dims = (20, 12, 9)
    t, w = ec.state(dims, "edges")
    slice_n = dims[0] * dims[1]
    p = ec.params(0.25, 2)
    with capi.Volume(ec.config(dims)) as whole:
        whole.upload(t, w)
        want = whole.extent(p).as_dict()
    with capi.Group(ec.config(dims), [0, 0, 0]) as group:
        for slab in group.slabs:
            a, b = slab.cfg.z_begin, slab.cfg.z_end
            slab.upload(t[a * slice_n:b * slice_n], w[a * slice_n:b * slice_n])
        got = group.extent(p).as_dict()
        gt, gw = group.download()
    print(f"group: {got}")
    assert got == want == es.extent(t, w, dims, band=0.25, margin=2)
    assert bits_equal(gt, t) and bits_equal(gw, w)


# ------------------------------------------------------------------------------------------------------------------------
# a batch: members of different dims, collected frames, one launch
# ------------------------------------------------------------------------------------------------------------------------
BATCH_DIMS = [(24, 18, 10), (40, 12, 7), (8, 8, 8)]


def batch_scene():
    """(configs, poses, depths): the three members centred on one optical axis around the scene of the first."""
    cfgs = [ec.config(d) for d in BATCH_DIMS]
    scene = synth.SurfScene(BATCH_DIMS[0], ec.VS, ec.origin_of(BATCH_DIMS[0]), K=ec.K_SMALL, h=ec.IM_HW[0], w=ec.IM_HW[1])
    poses = [scene.pose(k, n=8) for k in range(3)]
    return cfgs, poses, [scene.depth(c, quantize=True) for c in poses]


def test_batch_extents_in_one_launch(cuda):
    """Frames integrated with deferral on and not flushed by the test (three small members defer, and set_deferral(32) asks
    for it); the third member's mask is empty, so it stays fresh."""
    cfgs, poses, depths = batch_scene()
    d_dev = [cuda.from_numpy(d).cuda() for d in depths]
    masks = np.zeros((3,) + ec.IM_HW, np.uint8)
    masks[:2] = 255
    m_dev = cuda.from_numpy(masks).cuda()
    m_ptrs = [m_dev[i].data_ptr() for i in range(3)]
    p = ec.params(1.0, 2)
    with capi.Batch(cfgs) as batch:
        batch.volumes[0].set_deferral(32)
        for c2w, d in zip(poses, d_dev):
            batch.integrate_device(d.data_ptr(), m_ptrs, c2w)
        got = [e.as_dict() for e in batch.extents(p)]               # collected, not flushed
        single = [v.extent(p).as_dict() for v in batch.volumes]
        arrays = [v.download() for v in batch.volumes]
        again = [e.as_dict() for e in batch.extents(p)]
    for i, dims in enumerate(BATCH_DIMS):
        want = es.extent(*arrays[i], dims, margin=2)
        print(f"member {i} {dims}: {got[i]}")
        assert got[i] == single[i] == again[i] == want, (i, want)
    assert got[0]["n_surface"] > 0.1 * np.prod(BATCH_DIMS[0]) and got[1]["n_surface"] > 0.1 * np.prod(BATCH_DIMS[1])
    assert got[2] == es.empty(BATCH_DIMS[2])
    assert np.all(arrays[2][0] == 1.0) and np.all(arrays[2][1] == 0.0)


WIDE_BATCH_DIMS = [(24, 18, 10), (96, 88, 3), (66000, 4, 2)]


def test_batch_members_with_more_than_one_workgroup_per_slice(cuda):
    """The launch takes the largest member's workgroups per slice for every member (65 here), so the first member's further
    workgroups find no tile, and the partial records of the second and third member start behind those of the members before
    them."""
    assert [ec.workgroups_per_slice(d) for d in WIDE_BATCH_DIMS] == [1, 2, 65]
    p = ec.params(0.25, 1)
    with capi.Batch([ec.config(d) for d in WIDE_BATCH_DIMS]) as batch:
        for v, dims in zip(batch.volumes, WIDE_BATCH_DIMS):
            v.upload(*ec.state(dims, "random"))
        got = [e.as_dict() for e in batch.extents(p)]
        single = [v.extent(p).as_dict() for v in batch.volumes]
    for i, dims in enumerate(WIDE_BATCH_DIMS):
        want = es.extent(*ec.state(dims, "random"), dims, band=0.25, margin=1)
        print(f"member {i} {dims}: {got[i]}")
        assert got[i] == single[i] == want, (i, want)
        assert want["n_surface"] >= 0.10 * np.prod(dims) and min(want["border"]) > 0


# ------------------------------------------------------------------------------------------------------------------------
# the call only reads
# ------------------------------------------------------------------------------------------------------------------------
def test_extent_reads_only(cuda):
    """TSDF and weight bits are the same before and after a call, and a fused sequence integrated afterwards gives the bits it
    gives without the call: the free-space summary words, which those launches trust, were not touched."""
    dims = (72, 33, 17)
    poses, depths = ec.frames(dims)
    dev = [cuda.from_numpy(d).cuda() for d in depths]
    ptrs = [d.data_ptr() for d in dev]
    results = {}
    for with_call in (False, True):
        with capi.Volume(ec.config(dims)) as vol:
            vol.integrate_frames_device(ptrs[:2], poses[:2])
            if with_call:
                t0, w0 = vol.download()
                rec = vol.extent(ec.params(1.0, 1)).as_dict()
                t1, w1 = vol.download()
                assert bits_equal(t0, t1) and bits_equal(w0, w1)
                assert rec == es.extent(t0, w0, dims, margin=1) and rec["n_surface"] > 0
            vol.integrate_frames_device(ptrs[2:], poses[2:])
            results[with_call] = vol.download()
    assert bits_equal(results[True][0], results[False][0]) and bits_equal(results[True][1], results[False][1])
    assert not bits_equal(results[True][0], np.ones(int(np.prod(dims)), f32))


# ------------------------------------------------------------------------------------------------------------------------
# outgrown and moved
# ------------------------------------------------------------------------------------------------------------------------
def test_outgrown_object_moves_into_the_proposed_grid(cuda):
    """An object whose surface touches the x+ face of its (24, 18, 10) grid, on an exact lattice (tests/test_fuse_spec.py's
    lattice_shift_case: a power-of-two voxel size and origins that are multiples of it, so merging copies bits): the grid
    tsdf_extent_regrid proposes, created and merged into, holds the same surface voxels, shifted by lo_src - pad, none of them
    near a face."""
    from test_fuse_spec import VS, lattice_shift_case
    _, sg, t, w, _, _, _ = lattice_shift_case()
    sdims, so = sg[0], sg[1]
    t3, w3 = t.copy().reshape(sdims[::-1]), w.copy().reshape(sdims[::-1])
    for region in ((slice(None), slice(None), slice(0, 3)), (slice(None), slice(15, None), slice(None)), (slice(0, 2), slice(None), slice(None))):
        t3[region], w3[region] = 1.0, 0.0                            # fresh: x < 3, y >= 15, z < 2
    t, w = t3.ravel(), w3.ravel()
    scfg = fc.config(sdims, float(VS), so)
    p = capi.extent_params_default(scfg)
    pad = p.margin
    assert pad == 5
    with capi.Volume(scfg) as src:
        src.upload(t, w)
        e_src = src.extent(p)
        rec = e_src.as_dict()
        assert rec == es.extent(t, w, sdims, margin=pad)
        assert rec["border"][1] > 0 and rec["lo"] == [3, 0, 2] and rec["hi"] == [23, 14, 9]
        dcfg = capi.extent_regrid(scfg, e_src, pad, 4)
        assert (dcfg.dim_x, dcfg.dim_y, dcfg.dim_z) == (32, 28, 20)
        shift = [l - pad for l in rec["lo"]]
        assert bits_equal(np.array(dcfg.origin, f32), so + np.array(shift, f32) * f32(VS))
        with capi.Volume(dcfg) as dst:
            counts = dst.fuse_from(src)                               # the default parameters
            moved = dst.extent(p).as_dict()
    print(f"source {rec}\nmoved {moved}\ncounts {counts}")
    n = rec["n_surface"]
    assert moved["n_surface"] == n and counts["sampled"] >= n
    assert moved["lo"] == [l - s for l, s in zip(rec["lo"], shift)] == [pad] * 3
    assert moved["hi"] == [h - s for h, s in zip(rec["hi"], shift)]
    assert moved["sum"] == [v - n * s for v, s in zip(rec["sum"], shift)]
    assert moved["border"] == [0] * 6


# ------------------------------------------------------------------------------------------------------------------------
# refusals
# ------------------------------------------------------------------------------------------------------------------------
def test_refusals(cuda):
    lib = capi.load()
    dims = (16, 12, 8)
    cfg = fc.config(dims, 0.004, np.zeros(3, f32))
    out = (capi.Extent * 2)()
    bad_params = [(ec.params(thr=v), "weight_thresh") for v in (float("nan"), float("inf"), float("-inf"))]
    bad_params += [(ec.params(band=v), "band") for v in (float("nan"), float("inf"), 0.0, -0.5, 1.5)]
    bad_params += [(ec.params(margin=-1), "margin")]
    # 16 voxels of a grid 2^30 slices deep: 16 * (2^30)^2 = 2^64
    deep = capi.make_config((4, 4, 1 << 30), 0.004, np.zeros(3, f32), z_begin=5, z_end=6, K=fc.K_SMALL, im_height=fc.IM_HW[0],
                            im_width=fc.IM_HW[1])

    def refused(fn, who, h, p, o, word):
        rc = fn(h, C.byref(p) if p is not None else None, o)
        msg = lib.tsdf_last_error().decode()
        assert rc == -1 and who in msg and word in msg, (rc, msg, who, word)

    with capi.Volume(cfg) as vol, capi.Batch([cfg, cfg]) as batch, capi.Group(cfg, [0, 0]) as group, capi.Volume(deep) as slab:
        ok = ec.params(1.0, 1)
        for fn, who, h in ((lib.tsdf_volume_extent, "tsdf_volume_extent", vol._h), (lib.tsdf_batch_extents, "tsdf_batch_extents", batch._h),
                           (lib.tsdf_group_extent, "tsdf_group_extent", group._h)):
            refused(fn, who, None, ok, out, "NULL")
            refused(fn, who, h, None, out, "NULL")
            refused(fn, who, h, ok, None, "NULL")
            for p, word in bad_params:
                refused(fn, who, h, p, out, word)
        refused(lib.tsdf_volume_extent, "tsdf_volume_extent", slab._h, ok, out, "2^64")
        t, w = vol.download()                                         # nothing was touched, and the handles still work
        assert np.all(t == 1.0) and np.all(w == 0.0)
        assert vol.extent(ok).as_dict() == es.empty(dims)
        assert [e.as_dict() for e in batch.extents(ok)] == [es.empty(dims)] * 2
        assert group.extent(ok).as_dict() == es.empty(dims)
