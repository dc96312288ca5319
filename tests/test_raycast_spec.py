"""The raycasting rule (csrc/tsdf_raycast.hip.h, restated in tests/raycast_spec.py) means what it says, on the CPU:

  * volumes holding the exact truncated SDF of a plane and of a sphere (weights 1) render the analytic depth and normal;
  * a 96^3 S-surf volume fused by the CPU restatement of Integrate renders SurfScene's analytic depth within bounds measured
    here, at an integrated pose and halfway between two;
  * edge cases end within max_steps with the miss convention where nothing is hit;
  * tsdf_raycast_params_default and the tsdf_raycast_params layout (host only, no GPU).

The GPU tests (test_gpu_raycast.py) hold the device to this restatement bit for bit, so bounds set here hold there."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import raycast_spec as rs
from semantic_slam_amd import capi, synth

f32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EYE = np.eye(4, dtype=f32).ravel()
K_SMALL = np.array([200, 0, 80, 0, 200, 60, 0, 0, 1], f32)
HW_SMALL = (120, 160)


def grid_coords(dims, vs, origin):
    z, y, x = np.meshgrid(*[np.arange(d) for d in dims[::-1]], indexing="ij")
    return [np.float64(origin[i]) + vs * a.astype(np.float64) for i, a in enumerate((x, y, z))]


def tsdf_of(sdf, trunc):
    return np.clip(sdf / trunc, -1.0, 1.0).astype(f32).ravel()


# a 64^3 box of 1 cm voxels 0.5 m in front of the base camera, a plane facing it at z = 0.8 m
DIMS, VS, TRUNC = (64, 64, 64), 0.01, 0.05
ORIGIN = np.array([-0.32, -0.32, 0.5], f32)
PLANE_Z = 0.8


def plane_volume(weight=1.0):
    X, Y, Z = grid_coords(DIMS, VS, ORIGIN)
    t = tsdf_of(PLANE_Z - Z, TRUNC)
    return t, np.full(t.size, weight, f32)


def render(t, w, cam2base=EYE, K=K_SMALL, hw=HW_SMALL, near=0.0, far=6.0, thr=0.9, dims=DIMS, origin=ORIGIN, pixels=None):
    return rs.render(t, w, dims, origin, VS, TRUNC, K, hw, near, far, thr, cam2base, pixels=pixels)


def assert_miss_convention(o):
    m = ~o["hit"]
    assert np.all(o["depth"][m] == 0) and np.all(o["normal"][m] == 0)
    assert np.all(np.signbit(o["depth"][m]) == False)  # noqa: E712  (+0, not -0)


def assert_bounded(o, dims=DIMS):
    assert o["samples"].max() <= rs.max_steps(dims)


def camera_dirs(K, hw):
    h, w = hw
    v, u = np.mgrid[0:h, 0:w]
    return np.stack([(u - K[2]) / K[0], (v - K[5]) / K[4], np.ones((h, w))], -1).reshape(-1, 3).astype(np.float64)


# ------------------------------------------------------------------------------------------------------------------------
# analytic volumes
# ------------------------------------------------------------------------------------------------------------------------
def test_plane_depth_and_normal_are_analytic():
    t, w = plane_volume()
    o = render(t, w)
    d = camera_dirs(K_SMALL, HW_SMALL)
    hit_pt = d * PLANE_Z                                        # the analytic hit in the base (= camera) frame
    g = (hit_pt - ORIGIN.astype(np.float64)) / VS
    inside = np.all((g >= 2) & (g <= np.array(DIMS) - 3), axis=1)   # central differences need a voxel on each side
    assert inside.sum() > 10000
    assert np.all(o["hit"][inside])
    rel = np.abs(o["depth"][inside] - PLANE_Z) / PLANE_Z
    assert rel.max() < 1e-5, rel.max()
    n = o["normal"][inside]
    assert np.abs(n - np.array([0, 0, -1], f32)).max() < 1e-3     # toward the camera
    assert_miss_convention(o)
    assert_bounded(o)


def test_sphere_depth_and_normal_are_analytic():
    """Trilinear interpolation of a curved SDF is exact only to O(vs^2 / radius): for this 25-voxel radius the measured
    relative depth error is 1.9e-4 where the ray meets the surface within 25 degrees of its normal (cos > 0.9), 3.4e-4 within
    60 degrees, 8e-3 at grazing incidence.  The bounds below are those measurements with headroom; the plane's 1e-5 is the
    rule's own resolution where interpolation is exact."""
    X, Y, Z = grid_coords(DIMS, VS, ORIGIN)
    c, R = np.array([0.0, 0.0, 0.82]), 0.25
    t = tsdf_of(np.sqrt((X - c[0]) ** 2 + (Y - c[1]) ** 2 + (Z - c[2]) ** 2) - R, TRUNC)
    w = np.ones(t.size, f32)
    o = render(t, w)
    d = camera_dirs(K_SMALL, HW_SMALL)
    a, b, cc = (d * d).sum(1), -2 * d @ c, c @ c - R * R
    disc = b * b - 4 * a * cc
    z = np.where(disc >= 0, (-b - np.sqrt(np.maximum(disc, 0))) / (2 * a), 0)
    nrm = (d * z[:, None] - c) / R
    cosi = np.abs((nrm * d).sum(1)) / np.linalg.norm(d, axis=1)
    for lim, bound in ((0.9, 3e-4), (0.5, 6e-4)):
        m = (disc > 0) & (cosi > lim)
        assert m.sum() > 1000 and np.all(o["hit"][m])
        rel = np.abs(o["depth"][m] - z[m]) / z[m]
        assert rel.max() < bound, (lim, rel.max())
    m = (disc > 0) & (cosi > 0.5)
    ang = np.degrees(np.arccos(np.clip((o["normal"][m] * nrm[m]).sum(1), -1, 1)))
    assert ang.max() < 1.0, ang.max()
    assert_miss_convention(o)
    assert_bounded(o)


# ------------------------------------------------------------------------------------------------------------------------
# a fused volume against the analytic scene
# ------------------------------------------------------------------------------------------------------------------------
SURF_EDGE, SURF_VS = 96, 0.008
SCALE = 4                        # render at 160 x 120 with the TUM intrinsics scaled by 1/4


def scaled_K():
    K = synth.TUM_K.astype(np.float64).copy()
    K[[0, 2, 4, 5]] /= SCALE
    return K.astype(f32)


def away_from_edges(z, vs, px=3):
    """Pixels at least px pixels from a depth discontinuity (a jump of more than 2 voxels, or a hole)."""
    bad = z <= 0
    jump = np.zeros_like(bad)
    jump[:, 1:] |= np.abs(np.diff(z, axis=1)) > 2 * vs
    jump[1:, :] |= np.abs(np.diff(z, axis=0)) > 2 * vs
    bad = bad | jump
    out = bad.copy()
    for dy in range(-px, px + 1):
        for dx in range(-px, px + 1):
            out |= np.roll(np.roll(bad, dy, 0), dx, 1)
    return ~out


@pytest.fixture(scope="module")
def surf_volume(oracle):
    dims = (SURF_EDGE,) * 3
    origin = synth.surf_volume(SURF_EDGE, SURF_VS, 0.8)
    scene = synth.SurfScene(dims, SURF_VS, origin)
    t, w = oracle.init_grid(dims)
    trunc = float(f32(SURF_VS) * f32(5))
    for k in range(0, 64, 2):                                      # 32 frames of the 64-frame orbit
        c2w = scene.pose(k, n=64)
        oracle.integrate(synth.TUM_K, oracle.cam2base(EYE, c2w), scene.depth(c2w, quantize=True), dims, origin, SURF_VS,
                         trunc, t, w)
    return dims, origin, trunc, t, w


# measured on this restatement (median / p99 |depth error| in voxels, p99 angle to the analytic normal):
#   integrated pose k = 8:    0.0100 / 0.0702 vs, 1.21 deg
#   halfway pose k = 9:       0.0098 / 0.0680 vs, 1.26 deg
# the bounds are about 2x to 3x those
SURF_MEDIAN_VS, SURF_P99_VS, SURF_P99_DEG = 0.03, 0.15, 3.0


@pytest.mark.parametrize("k", [8, 9], ids=["integrated_pose", "halfway_pose"])
def test_fused_surf_volume_matches_the_scene(surf_volume, k):
    dims, origin, trunc, t, w = surf_volume
    K = scaled_K()
    hw = (480 // SCALE, 640 // SCALE)
    scene = synth.SurfScene(dims, SURF_VS, origin, K=K, h=hw[0], w=hw[1])
    c2w = scene.pose(k, n=64)
    want = scene.depth(c2w)                                       # unquantised, metres
    o = rs.render(t, w, dims, origin, SURF_VS, trunc, K, hw, 0.0, 6.0, 0.9, c2w)
    assert_bounded(o, dims)
    got = o["depth"].reshape(hw)
    T = np.asarray(c2w, np.float64).reshape(4, 4)
    dcam = camera_dirs(K, hw).reshape(hw + (3,))
    p_base = (dcam @ T[:3, :3].T) * want[..., None] + T[:3, 3]
    on_sphere = np.abs(np.linalg.norm(p_base - scene.center, axis=-1) - scene.radius) < 1e-6
    # the sphere only: SurfScene's back wall lies at the far face plus one voxel, outside the grid's sample range
    m = away_from_edges(want, SURF_VS) & (want > 0) & on_sphere
    assert m.sum() > 1500
    assert np.all(o["hit"].reshape(hw)[m])
    err = np.abs(got[m] - want[m]) / SURF_VS
    med, p99 = float(np.median(err)), float(np.percentile(err, 99))
    print(f"k={k}: median {med:.4f} vs, p99 {p99:.4f} vs")
    assert med < SURF_MEDIAN_VS and p99 < SURF_P99_VS, (med, p99)
    # analytic normal of the sphere, in the camera frame
    n_base = (p_base - scene.center) / np.linalg.norm(p_base - scene.center, axis=-1, keepdims=True)
    n_cam = n_base @ T[:3, :3]                                     # R^T n
    got_n = o["normal"].reshape(hw + (3,))
    mn = m & np.any(got_n != 0, axis=-1)
    assert mn.sum() > 0.9 * m.sum()
    ang = np.degrees(np.arccos(np.clip((got_n[mn] * n_cam[mn]).sum(-1), -1, 1)))
    p99a = float(np.percentile(ang, 99))
    print(f"k={k}: normal p99 {p99a:.3f} deg")
    assert p99a < SURF_P99_DEG, p99a


# ------------------------------------------------------------------------------------------------------------------------
# edge cases: every march ends within max_steps, misses follow the convention
# ------------------------------------------------------------------------------------------------------------------------
def test_camera_inside_the_box():
    t, w = plane_volume()
    c2b = synth.make_pose(np.eye(3), [0.0, 0.0, 0.6])              # 10 voxels inside the near face
    o = render(t, w, cam2base=c2b)
    assert_bounded(o)
    centre = (60 * 160 + 80)
    assert o["hit"][centre] and abs(o["depth"][centre] - (PLANE_Z - 0.6)) < 1e-6


def test_camera_facing_away():
    t, w = plane_volume()
    o = render(t, w, cam2base=synth.make_pose(synth.rot_y(math.pi), [0.0, 0.0, 0.3]))
    assert not o["hit"].any()
    assert_miss_convention(o)
    assert_bounded(o)


def test_axis_parallel_rays():
    """cx, cy on pixel centres and an identity rotation: the ray through (cx, cy) has gd_x = gd_y = 0 exactly."""
    t, w = plane_volume()
    K = np.array([200, 0, 80, 0, 200, 60, 0, 0, 1], f32)
    o = render(t, w, K=K, pixels=[(80, 60), (81, 60), (80, 61)])
    assert o["hit"].all() and abs(o["depth"][0] - PLANE_Z) < 1e-6
    # the same ray from a camera beside the box: always outside on x, a miss
    o = render(t, w, K=K, cam2base=synth.make_pose(np.eye(3), [1.0, 0.0, 0.0]), pixels=[(80, 60)])
    assert not o["hit"].any()
    assert_miss_convention(o)
    # and on the box's face x = 0 exactly: inside (0 <= go_x <= hi_x)
    c2b = synth.make_pose(np.eye(3), [float(ORIGIN[0]), 0.0, 0.0])
    o = render(t, w, K=K, cam2base=c2b, pixels=[(80, 60)])
    assert_bounded(o)


def test_singular_rotation():
    """R = 0 (what a singular base2world composes to): every gd is 0, the ray stays on one point; a miss, bounded."""
    t, w = plane_volume()
    c2b = np.zeros(16, f32)
    c2b[15] = 1
    for T in ([0.0, 0.0, 0.0], [0.0, 0.0, 0.7], [0.0, 0.0, 0.9]):   # outside; inside in front of the plane; behind it
        c2b[[3, 7, 11]] = T
        o = render(t, w, cam2base=c2b)
        assert not o["hit"].any()
        assert_miss_convention(o)
        assert_bounded(o)


def test_non_finite_and_signed_zero_values():
    rng = np.random.default_rng(5)
    t, w = plane_volume()
    idx = rng.choice(t.size, 4000, replace=False)
    t[idx[:1000]] = np.nan
    t[idx[1000:2000]] = np.inf
    t[idx[2000:3000]] = -np.inf
    t[idx[3000:3500]] = -0.0
    t[idx[3500:]] = 0.0
    o = render(t, w)
    assert_bounded(o)
    assert np.all(np.isfinite(o["depth"])) and np.all(np.isfinite(o["normal"]))
    assert o["hit"].sum() > 1000
    assert_miss_convention(o)


def test_weights_at_and_above_the_threshold():
    thr = f32(0.9)
    t, _ = plane_volume()
    o = render(t, np.full(t.size, thr, f32), thr=thr)
    assert not o["hit"].any()
    assert_miss_convention(o)
    assert_bounded(o)
    o = render(t, np.full(t.size, np.nextafter(thr, f32(2)), f32), thr=thr)
    assert o["hit"].sum() > 10000


def test_near_beyond_the_box_and_far_inside_it():
    t, w = plane_volume()
    far_face = float(ORIGIN[2]) + VS * (DIMS[2] - 1)
    o = render(t, w, near=far_face + 0.01, far=6.0)
    assert not o["hit"].any()
    assert_miss_convention(o)
    o = render(t, w, near=0.0, far=PLANE_Z - 0.05)                 # the march stops before the plane
    assert not o["hit"].any()
    assert_miss_convention(o)
    assert_bounded(o)
    o = render(t, w, near=0.0, far=PLANE_Z + 0.05)
    assert o["hit"].sum() > 10000


# ------------------------------------------------------------------------------------------------------------------------
# host-only ABI pieces
# ------------------------------------------------------------------------------------------------------------------------
def test_raycast_params_default():
    cfg = capi.make_config((64, 48, 32), 0.01, [0, 0, 0], K=K_SMALL, im_height=120, im_width=160, max_depth=4.5)
    p = capi.raycast_params_default(cfg)
    assert list(p.cam_K) == list(K_SMALL)
    assert (p.im_height, p.im_width) == (120, 160)
    assert p.near_m == 0.0 and p.far_m == f32(4.5) and p.weight_thresh == f32(0.9)
    assert capi.load().tsdf_raycast_params_default(None, C.byref(p)) == -1


def test_raycast_params_layout_matches_c(tmp_path):
    prog = tmp_path / "layout.c"
    fields = [f for f, _ in capi.RaycastParams._fields_]
    body = "\n".join(f'printf("{f} %zu\\n", offsetof(tsdf_raycast_params, {f}));' for f in fields)
    prog.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "tsdf_hip.h"\n'
                    'int main(void){printf("size %zu\\n", sizeof(tsdf_raycast_params));\n' + body + "\nreturn 0;}\n")
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(prog), "-o", str(exe)])
    got = dict(line.split() for line in subprocess.check_output([str(exe)]).decode().splitlines())
    assert int(got["size"]) == C.sizeof(capi.RaycastParams)
    for f in fields:
        assert int(got[f]) == getattr(capi.RaycastParams, f).offset, f
