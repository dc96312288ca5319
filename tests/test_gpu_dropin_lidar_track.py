"""Drop-in proof for scan tracking: a C++ program written against include/tsdf.hpp as the reference's lidar labeller drives its
TSDF member (tests/dropin_lidar_track.cpp) asks the object for the pose of a scan (TSDF::TrackScan) and gets, bit for bit, the
pose composed from tsdf_scan_track through capi.py; a lost track returns false and leaves the caller's pose as it was; with
TSDF::SetScanGround on the answer is that of the drop_flag = 1 call on tsdf_scan_mark_ground's flags."""
import os
import struct
import subprocess

import numpy as np
import pytest

import scan_ground_spec as sg
import scan_track_cases as sc
import scan_track_spec as sts
from semantic_slam_amd import capi

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "semantic_slam_amd")
F = np.float32
# scanner (x forward, y left, z up) to camera (x right, y down, z forward), a lever arm between them
VELO2CAM = np.array([[0, -1, 0, 0.05], [0, 0, -1, -0.08], [1, 0, 0, -0.27], [0, 0, 0, 1]], F)


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("dropin_lidar_track") / "dropin_lidar_track")
    subprocess.check_call(["g++", "-O1", "-std=c++11", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "dropin_lidar_track.cpp"), "-o", exe,
                           "-L", PKG, "-ltsdf_dropin", "-ltsdf_hip", f"-Wl,-rpath,{PKG}"])
    return exe


def cam_pose(velo2world):
    """cam2world = velo2world * inverse(velo2cam), the library's host helpers."""
    ok, inv = capi.invert_matrix(VELO2CAM)
    assert ok
    return capi.multiply_matrix(velo2world, inv)


def test_lidar_callsite_tracks_the_scan(cuda, harness, tmp_path):
    cfg = sc.corner_config(sc.BIG)
    pts, truth = sc.corner_scan(sc.BIG)
    frames = sc.corner_frames(sc.BIG)
    b2w = np.asarray(cfg.base2world, np.float64).reshape(4, 4)
    poses = [(b2w @ c2b).astype(F).ravel() for _, c2b in frames]
    inside = cam_pose(sc.moved(truth, 1.0, 0.3, 13))
    outside = cam_pose(sc.shifted(truth, (2.2, 2.2, -2.2)))            # every plane off by more than the truncation distance
    g = sg.to_capi(sc.ground_params())
    assert F(cfg.trunc_margin) == F(cfg.voxel_size) * F(5)              # what the harness sets
    inp = tmp_path / "frames.bin"
    with open(inp, "wb") as f:
        f.write(struct.pack("<7i", cfg.im_height, cfg.im_width, len(frames), *sc.DIMS, len(pts)))
        f.write(struct.pack("<2f", cfg.voxel_size, cfg.max_depth))
        for a in (cfg.origin, cfg.cam_K, cfg.base2world, VELO2CAM):
            f.write(np.ascontiguousarray(a, F).tobytes())
        f.write(bytes(g))
        for (depth, _), c2w in zip(frames, poses):
            f.write(c2w.tobytes())
            f.write(depth.tobytes())
        f.write(pts.tobytes())
        f.write(inside.tobytes())
        f.write(outside.tobytes())
    out = subprocess.run([harness, str(inp)], cwd=str(tmp_path), capture_output=True, text=True)
    assert out.returncode == 0 and "done" in out.stdout, out.stderr
    raw = (tmp_path / "results.bin").read_bytes()
    assert len(raw) == 5 * 68
    calls = [(struct.unpack_from("<i", raw, 68 * k)[0], np.frombuffer(raw, F, 16, 68 * k + 4)) for k in range(5)]

    # the same calls through capi.py
    with capi.Volume(cfg) as v, capi.Scanner(cfg.im_height, cfg.im_width) as scanner:
        for (depth, _), c2w in zip(frames, poses):
            v.integrate(depth, c2w)
        p = capi.scan_track_params_default(cfg)
        guess = capi.multiply_matrix(inside, VELO2CAM)
        v2w, st = v.track_scan(pts, guess, params=p)
        _, st_out = v.track_scan(pts, capi.multiply_matrix(outside, VELO2CAM), params=p)
        flags, _, _, _ = scanner.mark_ground(pts, g, want_state=False, want_winner=False, want_counts=False)
        p.drop_flag = 1
        v2w_ground, st_ground = v.track_scan(pts, guess, params=p, flags=flags)
        _, st_none = v.track_scan(np.zeros((0, 4), F), guess)
    assert st["status"] != 2 and st["pairs"] > 1000 and st_out["status"] == 2 and st_none["status"] == 2
    assert st_ground["status"] != 2 and (flags == 1).sum() > 1000 and st_ground["pairs"] < st["pairs"]
    want, want_ground = cam_pose(v2w.ravel()), cam_pose(v2w_ground.ravel())
    assert calls[0][0] == 1 and calls[0][1].tobytes() == want.tobytes()
    assert calls[1][0] == 0 and calls[1][1].tobytes() == outside.tobytes(), "a lost track leaves cam2world_vec as it was"
    assert calls[2][0] == 1 and calls[2][1].tobytes() == want_ground.tobytes() and want_ground.tobytes() != want.tobytes()
    assert calls[3][0] == 1 and calls[3][1].tobytes() == want.tobytes()
    assert calls[4][0] == 0 and calls[4][1].tobytes() == inside.tobytes()
    # and the refined pose is nearer the truth than the guess
    r0, t0 = sts.pose_error(guess, truth)
    r1, t1 = sts.pose_error(v2w, truth)
    print(f"TrackScan: {r0:.3f} deg {1e3 * t0:.1f} mm -> {r1:.3f} deg {1e3 * t1:.1f} mm from the truth; {st}")
    assert r1 < r0 and t1 < t0
