"""class TSDFfusion estimating its own poses (include/TSDFfusion.hpp: EstimatePose, Pose, LastTrackStatus): a short textured
sequence inside the class's [0, 10]^3 m volume, SetPose for the first frame only, pose-less Integrate calls after it
(tests/dropin_tsdffusion_track.cpp).  The poses the class reports equal, bit for bit, those of the same call sequence made
through capi.py -- track_rgbd from the last pose, then integrate_rgbd (integrate without a colour image) at the estimate; an
all-zero depth frame is lost, is not integrated and leaves the pose unchanged; with EstimatePose off the class uses the pose
as set and tracks nothing."""
import os
import struct
import subprocess

import numpy as np
import pytest

import photo_cases as pc
import track_spec as ts
from semantic_slam_amd import capi, synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "semantic_slam_amd")
f32 = np.float32
HW = (480, 640)
LOST_AT = 3          # the frame whose depth is all zero


def sequence():
    """[(true pose, depth, rgb)]: a sphere in front of a wall 2.5 to 4.5 m ahead, textured at four times photo_cases' wavelengths
    (0.4 m and up: 20 voxel edges of 0.02 m), seen from a camera that drifts 2 cm and 0.3 degrees a frame."""
    scene = synth.SurfScene((200, 200, 200), 0.02, np.array([3.0, 3.0, 3.0], f32))
    K = synth.TUM_K.astype(np.float64)
    vv, uu = np.mgrid[0:HW[0], 0:HW[1]]
    rays = np.stack([(uu - K[2]) / K[0], (vv - K[5]) / K[4], np.ones(HW)], axis=-1)
    out = []
    for k in range(5):
        pose = synth.make_pose(synth.rot_y(0.005 * k), [5.0 + 0.02 * k, 5.0 - 0.01 * k, 0.5])
        depth = scene.depth(pose, quantize=True)
        T = np.asarray(pose, np.float64).reshape(4, 4)
        P = (rays * depth[..., None].astype(np.float64)) @ T[:3, :3].T + T[:3, 3]
        rgb = np.where((depth > 0)[..., None], pc.texture(P * 0.25), 0).astype(np.uint8)
        if k == LOST_AT:
            depth = np.zeros(HW, f32)
        out.append((np.asarray(pose, f32).ravel(), np.ascontiguousarray(depth, f32), np.ascontiguousarray(rgb)))
    return out


def run_class(tmp_path, frames, estimate, with_rgb):
    exe = str(tmp_path / "dropin_tsdffusion_track")
    subprocess.check_call(["g++", "-O1", "-std=c++11", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "dropin_tsdffusion_track.cpp"), "-o", exe,
                           "-L", PKG, "-ltsdf_dropin", "-ltsdf_hip", f"-Wl,-rpath,{PKG}"])
    inp, out = tmp_path / "frames.bin", tmp_path / "poses.bin"
    with open(inp, "wb") as f:
        f.write(struct.pack("<iii", len(frames), int(estimate), int(with_rgb)))
        f.write(frames[0][0].tobytes())
        for _, d, rgb in frames:
            f.write(d.tobytes())
            f.write(rgb.tobytes())
    subprocess.check_call([exe, str(inp), str(out)], cwd=str(tmp_path))
    raw = out.read_bytes()
    assert len(raw) == len(frames) * 68
    return [(struct.unpack_from("<i", raw, 68 * k)[0], np.frombuffer(raw, f32, 16, 68 * k + 4).copy()) for k in range(len(frames))]


def run_capi(frames, with_rgb):
    """The same calls through capi.py on the class's volume (ref: src/TSDFfusion.py.in:19-29)."""
    cfg = capi.make_config((500, 500, 500), 0.02, [0, 0, 0])
    out = []
    with capi.Volume(cfg) as vol:
        vol.colour_enable()
        pose = frames[0][0].copy()
        for k, (_, d, rgb) in enumerate(frames):
            status = -1
            if k > 0:
                est, st = vol.track_rgbd(d, rgb if with_rgb else None, pose)
                status = st["status"]
                if status != 2:
                    pose = est.ravel().copy()
            if status != 2:
                if with_rgb:
                    vol.integrate_rgbd(d, rgb, pose)
                else:
                    vol.integrate(d, pose)
            out.append((status, pose.copy(), st if k > 0 else None))
    return out


@pytest.mark.parametrize("with_rgb", [True, False], ids=["rgb", "depth_only"])
def test_the_class_tracks_as_the_c_abi_does(cuda, tmp_path, with_rgb):
    frames = sequence()
    got = run_class(tmp_path, frames, True, with_rgb)
    want = run_capi(frames, with_rgb)
    for k, ((gs, gp), (ws, wp, st)) in enumerate(zip(got, want)):
        assert gs == ws, (k, gs, ws)
        assert gp.tobytes() == wp.tobytes(), f"frame {k}: the class's pose differs from the C ABI's"
    assert got[0][0] == -1 and got[0][1].tobytes() == frames[0][0].tobytes()          # the first frame: the pose as set
    assert got[LOST_AT][0] == 2 and got[LOST_AT][1].tobytes() == got[LOST_AT - 1][1].tobytes()
    for k in (1, 2, 4):
        assert (want[k][2]["photo_pairs"] > 10000) == with_rgb
        e = ts.pose_error(got[k][1], frames[k][0])
        print(f"frame {k}: status {got[k][0]}, {e[0] * 1e3:.2f} mm / {e[1]:.2e} rad from the truth")
        if with_rgb:
            # (one sphere in front of a wall leaves depth alone a free rotation: test_track_spec.py; its poses are only compared)
            assert got[k][0] in (0, 1), (k, got[k][0])
            # tracking must beat standing still: a frame moves the camera 2.2 cm and 5e-3 rad
            assert e[0] < 0.0224 and e[1] < 5e-3, (k, e)


def test_with_estimation_off_the_class_ignores_it(cuda, tmp_path):
    frames = sequence()[:3]
    got = run_class(tmp_path, frames, False, True)
    for status, pose in got:
        assert status == -1 and pose.tobytes() == frames[0][0].tobytes()
