"""The parity cases of tests/test_gpu_fuse.py (test infrastructure): destination and source configurations, seeded rigid
transforms and uploaded states, with the restatement's result computed once per case and shared.  tests/test_fuse_spec.py
checks on the CPU that no case is vacuous."""
import functools

import numpy as np

import fuse_spec as fs
from fuzz_cases import NAN_PAYLOAD, edge_values
from semantic_slam_amd import capi, synth

f32 = np.float32
IM_HW = (120, 160)
K_SMALL = synth.TUM_K.copy()
K_SMALL[[0, 2, 4, 5]] *= 0.25          # the TUM camera at a quarter of its resolution
# odd rows (the per-voxel path); 16-byte rows, more than one workgroup per axis; 16-byte rows whose last x tile (8 quads) is partial
DST_SHAPES = [(37, 22, 13), (64, 48, 40), (44, 12, 9)]
SRC_SHAPE = (24, 33, 17)
DST_VS, SRC_VS = 0.004, 0.005
N_POSES = 3
STATES = ["surf", "edges"]
WEIGHT_THRESH = 0.9


def config(dims, vs, origin, trunc=None, base2world=None):
    return capi.make_config(dims, vs, origin, trunc=trunc, K=K_SMALL, base2world=base2world, im_height=IM_HW[0],
                            im_width=IM_HW[1])


def configs(dst_dims, pose):
    """Destination: 4 mm voxels, truncation 20 mm, base frame = world.  Source: 5 mm voxels, truncation 25 mm (ratio 1.25) or,
    for pose 1, 15 mm (ratio 0.75); its box is centred on the destination's and then moved by the pose's seeded rigid
    transform (pose 2 also shifts it by about a quarter of its size, so that it leaves the destination on one side)."""
    d_ext, s_ext = np.array(dst_dims) * DST_VS, np.array(SRC_SHAPE) * SRC_VS
    centre = np.array([0.0, 0.0, 0.9 + d_ext[2] / 2])
    d_origin = (centre - d_ext / 2).astype(f32)
    s_origin = (centre - s_ext / 2).astype(f32)
    rng = np.random.default_rng(100 + pose)
    ax, ay, az = rng.uniform(-0.25, 0.25, 3)
    R = synth.rot_z(az) @ synth.rot_y(ay) @ synth.rot_x(ax)
    shift = rng.uniform(-0.004, 0.004, 3) + (np.array([0.03, 0.02, 0.01]) if pose == 2 else 0.0)
    b2w = fs.pose_about(R, centre, shift)
    s_trunc = 0.015 if pose == 1 else 0.025
    return config(dst_dims, DST_VS, d_origin), config(SRC_SHAPE, SRC_VS, s_origin, trunc=s_trunc, base2world=b2w)


def surf_states(oracle, dcfg, scfg):
    """One scene (synth.SurfScene: a sphere and a back wall, sized by the source's box where it sits before the transform
    moves it; the destination's frame is the world) fused into both grids through the CPU oracle: the source from
    four views, the destination from two of them with the right 45 % of the image missing, so part of it is fresh."""
    ddims, d_origin, d_vs, d_trunc, d_b2w = fs.grid_of(dcfg)
    sdims, s_origin, s_vs, s_trunc, s_b2w = fs.grid_of(scfg)
    scene = synth.SurfScene(sdims, float(s_vs), s_origin, K=K_SMALL, h=IM_HW[0], w=IM_HW[1])   # the source's box, not moved
    dt, dw = oracle.init_grid(ddims)
    st, sw = oracle.init_grid(sdims)
    for k in range(4):
        c2w = scene.pose(k, n=8)
        depth = scene.depth(c2w, quantize=True)
        oracle.integrate(K_SMALL, oracle.cam2base(s_b2w, c2w), depth, sdims, s_origin, float(s_vs), float(s_trunc), st, sw)
        if k < 2:
            part = depth.copy()
            part[:, int(0.55 * IM_HW[1]):] = 0.0
            oracle.integrate(K_SMALL, oracle.cam2base(d_b2w, c2w), part, ddims, d_origin, float(d_vs), float(d_trunc), dt, dw)
    return dt, dw, st, sw


def edge_states(seed, n_dst, n_src):
    """Random values with NaN (payload), +-inf, +-0, +-1 as TSDF and weights at the threshold, one ulp above it, NaN, -1 and
    0 (fuzz_cases.edge_values): few of them in the source, where one bad corner of eight rejects a sample, many in the
    destination, 30 % of which is fresh (1, 0)."""
    rng = np.random.default_rng(seed)
    st, sw = edge_values(rng, n_src, WEIGHT_THRESH, p_special=0.03, p_weight=0.06)
    dt, dw = edge_values(rng, n_dst, WEIGHT_THRESH, p_special=0.25, p_weight=0.3)
    fresh = rng.uniform(0, 1, n_dst) < 0.3
    dt[fresh], dw[fresh] = 1.0, 0.0
    assert np.any(dt.view(np.uint32) == NAN_PAYLOAD.view(np.uint32)) and np.any(st.view(np.uint32) == NAN_PAYLOAD.view(np.uint32))
    return dt, dw, st, sw


@functools.lru_cache(maxsize=None)
def parity_case(dst_dims, pose, state):
    """(dst cfg, src cfg, (dst t, dst w, src t, src w), (want t, want w, want counts), info) -- computed once, not to be
    changed by its users."""
    from oracle.oracle import Oracle
    dcfg, scfg = configs(dst_dims, pose)
    if state == "surf":
        arrays = surf_states(Oracle(), dcfg, scfg)
    else:
        arrays = edge_states(7 * pose + len(dst_dims) + dst_dims[0], int(np.prod(dst_dims)), int(np.prod(SRC_SHAPE)))
    info = {}
    want = fs.fuse(arrays[0], arrays[1], fs.grid_of(dcfg), arrays[2], arrays[3], fs.grid_of(scfg),
                   weight_thresh=WEIGHT_THRESH, agree_tol=0.4, write=1, info=info)
    for a in arrays + want[:2]:
        a.setflags(write=False)
    return dcfg, scfg, arrays, want, info


def vacuity(dst_dims, pose, state):
    """(fraction of destination voxels sampled, fraction inside the source box but rejected or skipped, voxels updated as
    fresh, voxels updated as observed) of a case."""
    _, _, _, want, info = parity_case(dst_dims, pose, state)
    n = int(np.prod(dst_dims))
    return (want[2]["sampled"] / n, int((info["inside"] & ~info["valid"]).sum()) / n, info["fresh"], info["observed"])
