"""The edges of the launch geometry (csrc/launch_geometry.h) on the device: slabs of at most 512 x 13 x 3 voxels whose every
rounded-up division has a remainder -- rows that are no quads, six chunks in two workgroups, nine rows at one and two segments
per row, three slices under bricks of two, row groups of four over 13 and 9 rows -- driven through each mapping the product
launches and compared with the oracle bit for bit after download.  The small camera and the scene of tests/walk_cases.py,
three frames; the references are computed once per shape and shared, read-only."""
import functools

import numpy as np
import pytest

import walk_cases as wc
from semantic_slam_amd import capi

pytestmark = pytest.mark.gpu

N_FRAMES = 3
# dims, voxel size (the grid about 1.2 m wide), the mapping of a one-frame launch, the brick of the classified launches:
# 2 quads x 4 rows x 2 slices where two quads divide the row's, else 5 x 4 x 2 (100 voxels are 25 quads)
SHAPES = {
    "scalar": dict(dims=(37, 5, 3), vs=0.03, brick=None),         # rows not divisible into quads
    "flat": dict(dims=(100, 13, 3), vs=0.012, brick=(5, 4, 2)),   # 6 chunks, 2 workgroups
    "rows1": dict(dims=(256, 9, 3), vs=0.005, brick=(2, 4, 2)),   # nseg 1, 9 rows
    "rows2": dict(dims=(512, 9, 3), vs=0.0025, brick=(2, 4, 2)),  # nseg 2, 9 rows
}
QUAD_SHAPES = [s for s in SHAPES if SHAPES[s]["brick"]]


def geometry(shape):
    s = SHAPES[shape]
    return s["dims"], s["vs"], wc.origin_of(s["dims"], s["vs"])


def frames(shape):
    dims, vs, _ = geometry(shape)
    return [wc.scene_frame(dims, vs, k, True) for k in range(N_FRAMES)]


def mask_of(member):
    """An instance mask over part of the image: the left two thirds (member 0) or the lower right (member 1)."""
    m = np.zeros(wc.IM_HW, np.uint8)
    if member == 0:
        m[:, :2 * wc.IM_HW[1] // 3] = 255
    else:
        m[wc.IM_HW[0] // 3:, wc.IM_HW[1] // 4:] = 255
    m.setflags(write=False)
    return m


@functools.lru_cache(maxsize=None)
def reference(oracle, shape, member):
    """(tsdf, weight) of the oracle after the shape's three frames, each times the member's mask (member None: unmasked)."""
    dims, vs, origin = geometry(shape)
    cfg = wc.config(dims, vs, origin)
    t, w = oracle.init_grid(dims)
    for c2w, depth in frames(shape):
        d = depth if member is None else oracle.mask_depth(depth, mask_of(member))
        oracle.integrate(wc.K_SMALL, oracle.cam2base(np.eye(4, dtype=np.float32), c2w), d, dims, origin, vs, cfg.trunc_margin, t, w)
    t.setflags(write=False)
    w.setflags(write=False)
    return t, w


def same_as_reference(oracle, vol, shape, member):
    rt, rw = reference(oracle, shape, member)
    t, w = vol.download()
    assert np.array_equal(w, rw), f"{shape}: weights differ at {np.flatnonzero(w != rw)[:8]}"
    assert np.array_equal(t.view(np.uint32), rt.view(np.uint32)), f"{shape}: TSDF differs"
    assert rw.sum() > 0, "the frames must touch the slab"


def classified(vol, shape):
    vol.set_kernel_variant(8)
    vol.set_brick_shape(*SHAPES[shape]["brick"])


def on_device(cuda, array):
    return cuda.from_numpy(np.array(array)).cuda()      # (a copy: the shared frames and masks are read-only)


def volume(shape):
    dims, vs, origin = geometry(shape)
    return capi.Volume(wc.config(dims, vs, origin))


@pytest.mark.parametrize("shape", list(SHAPES))
def test_one_frame_per_call(cuda, oracle, shape):
    with volume(shape) as vol:
        vol.set_deferral(0)
        keep = []
        for c2w, depth in frames(shape):
            keep.append(on_device(cuda, depth))
            vol.integrate_device(keep[-1].data_ptr(), c2w)
        same_as_reference(oracle, vol, shape, None)


@pytest.mark.parametrize("variant", [7, 8])
@pytest.mark.parametrize("shape", QUAD_SHAPES)
def test_fused_sequence(cuda, oracle, shape, variant):
    with volume(shape) as vol:
        if variant == 8:
            classified(vol, shape)
        else:
            vol.set_kernel_variant(variant)
        fr = frames(shape)
        keep = [on_device(cuda, depth) for _, depth in fr]
        vol.integrate_frames_device([d.data_ptr() for d in keep], np.stack([c2w for c2w, _ in fr]))
        same_as_reference(oracle, vol, shape, None)


@pytest.mark.parametrize("shape", QUAD_SHAPES)
def test_masked_one_frame_classified(cuda, oracle, shape):
    with volume(shape) as vol:
        classified(vol, shape)
        vol.set_deferral(0)
        m_dev = on_device(cuda, mask_of(0))
        keep = []
        for c2w, depth in frames(shape):
            keep.append(on_device(cuda, depth))
            vol.integrate_masked_device(keep[-1].data_ptr(), m_dev.data_ptr(), c2w)
        same_as_reference(oracle, vol, shape, 0)


@pytest.mark.parametrize("deferred", [False, True])
@pytest.mark.parametrize("shape", QUAD_SHAPES)
def test_batch_of_two_masked_members(cuda, oracle, shape, deferred):
    dims, vs, origin = geometry(shape)
    with capi.Batch([wc.config(dims, vs, origin), wc.config(dims, vs, origin)]) as batch:
        for vol in batch.volumes:
            classified(vol, shape)
        if not deferred:
            batch.volumes[0].set_deferral(0)
        m_dev = [on_device(cuda, mask_of(i)) for i in range(2)]
        keep = []
        for c2w, depth in frames(shape):
            keep.append(on_device(cuda, depth))
            batch.integrate_device(keep[-1].data_ptr(), [m.data_ptr() for m in m_dev], c2w)
        for i, vol in enumerate(batch.volumes):
            same_as_reference(oracle, vol, shape, i)
