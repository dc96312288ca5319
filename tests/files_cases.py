"""The inputs of tests/test_mesh_files.py (CPU) and tests/test_gpu_files.py (test infrastructure): one small fused, coloured
scene -- the third shape of tests/test_gpu_colour.py -- and a hand-made triangle soup for the corners of the formats."""
import functools

import numpy as np

from semantic_slam_amd import capi, synth

f32 = np.float32
DIMS, VS = (36, 20, 12), 0.03
ORIGIN = synth.surf_volume(36, VS, 0.7)
Z_CUT = 5                      # the second handle holds z in [Z_CUT, 12) and gets no halo


def config(z_begin=0, z_end=None):
    return capi.make_config(DIMS, VS, ORIGIN, z_begin=z_begin, z_end=z_end)


@functools.lru_cache(maxsize=None)
def frames():
    """[(pose, depth, rgb)]: three views, quantized depth, the images of tests/test_gpu_colour.py."""
    from test_gpu_colour import images
    scene = synth.SurfScene(DIMS, VS, ORIGIN)
    out = []
    for k in range(3):
        pose = scene.pose(k, 7)
        out.append((pose, scene.depth(pose, quantize=True), images(480, 640, k)))
    return out


@functools.lru_cache(maxsize=None)
def oracle_state():
    """(tsdf, weight, colour) of the whole grid after the three frames, by the oracle; shared, not to be written to."""
    from oracle.oracle import Oracle
    orc = Oracle()
    cfg = config()
    t, w = orc.init_grid(DIMS)
    c = np.zeros(t.size, np.uint32)
    for pose, depth, rgb in frames():
        orc.integrate(cfg.cam_K, pose, depth, DIMS, ORIGIN, VS, cfg.trunc_margin, t, w)
        orc.integrate_colour(cfg.cam_K, pose, depth, rgb, DIMS, ORIGIN, VS, cfg.trunc_margin, w, c)
    for a in (t, w, c):
        a.setflags(write=False)
    return t, w, c


def oracle_mesh(z_begin=0):
    """(triangles [n, 3, 3], colour of the slab) of the slab [z_begin, 12), without a halo."""
    from oracle.oracle import Oracle
    t, w, c = oracle_state()
    first = z_begin * DIMS[0] * DIMS[1]
    tri = Oracle().mesh_triangles(np.ascontiguousarray(t[first:]), np.ascontiguousarray(w[first:]), DIMS[:2], z_begin, DIMS[2], VS, ORIGIN)
    return tri, np.ascontiguousarray(c[first:])


# ---- the hand-made soup ----------------------------------------------------------------------------------------------------
HAND_DIMS, HAND_VS, HAND_ORIGIN, HAND_Z = (6, 5, 8), f32(0.25), np.array([-0.5, 0.25, 1.0], f32), (2, 7)


def hand_soup():
    """(triangles, colour of the slab): voxel coordinates i map to origin + i * 0.25, all exact in float32, so a vertex given
    at i + 0.5 sits exactly halfway between two voxels.  In voxel units, per axis: outside the grid below and above (the clamp
    runs on both sides; in z the slab is [2, 7) of 8 slices, so z = 1 and z = 7 are inside the grid and outside the slab);
    exact halves, positive (2.5 -> 3) and negative (-0.5 -> -1, clamped to 0; -1.5 -> -2); a zero-area triangle whose
    vertices no other face touches (normal (0, 0, 0)); two triangles that share an edge; two vertices that differ only in the
    sign of a zero (origin x is -0.5, so voxel 2 is x = +0.0: one is written as -0.0) and stay distinct."""
    def p(i, j, k):
        return HAND_ORIGIN + np.array([i, j, k], f32) * HAND_VS
    tri = np.array([
        [p(0, 0, 2), p(3, 0, 2), p(0, 3, 2)],                    # inside; shares the edge (3,0,2)-(0,3,2) with the next
        [p(3, 0, 2), p(3, 3, 4), p(0, 3, 2)],
        [p(-3, -2, 1), p(9, 1, 3), p(1, 8, 7)],                  # below and above the grid in x and y, the slab in z
        [p(2.5, 1.5, 3.5), p(-0.5, -1.5, 4.5), p(0.5, 3.5, -2.5)],   # exact halves of both signs
        [p(4, 4, 5), p(4, 4, 5), p(5, 4, 6)],                    # zero area, touching nothing else
        [p(2, 1, 3), p(2, 2, 3), p(1, 1, 4)],                    # x = +0.0 ...
        [p(2, 1, 3), p(2, 2, 3), p(1, 2, 4)],                    # ... and the same two vertices with x = -0.0
    ], f32)
    assert tri[5, 0, 0] == 0.0 and not np.signbit(tri[5, 0, 0])
    tri[6, 0, 0] = tri[6, 1, 0] = f32(-0.0)
    rng = np.random.default_rng(5)
    colour = rng.integers(0, 1 << 24, (HAND_Z[1] - HAND_Z[0]) * HAND_DIMS[1] * HAND_DIMS[0], dtype=np.uint32)
    return tri, colour
