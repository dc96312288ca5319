"""Drop-in proof for the ground marking: a C++ program written against include/tsdf.hpp as the reference's lidar labeller drives
its TSDF member (tests/dropin_lidar_ground.cpp), with TSDF::SetScanGround and TSDF::SetScanFill set, writes the files the same
calls through capi.py write -- byte for byte, on one device and with the grid cut into two z-slabs -- and after ClearScanGround
the files of an object that never set it."""
import os
import struct
import subprocess

import numpy as np
import pytest

import scan_cases
import scan_ground_cases as cases
import scan_ground_spec as spec
from semantic_slam_amd import capi

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "semantic_slam_amd")
F = np.float32
FILL = (5, 8, 0.05)


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("dropin_lidar_ground") / "dropin_lidar_ground")
    subprocess.check_call(["g++", "-O1", "-std=c++11", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "dropin_lidar_ground.cpp"), "-o", exe,
                           "-L", PKG, "-ltsdf_dropin", "-ltsdf_hip", f"-Wl,-rpath,{PKG}"])
    return exe


def config():
    return capi.make_config(scan_cases.FUSE_DIMS, scan_cases.FUSE_VS, scan_cases.FUSE_ORIGIN, K=scan_cases.FUSE_K,
                            im_height=scan_cases.FUSE_H, im_width=scan_cases.FUSE_W)


@pytest.mark.parametrize("layout", ["single", "slabs"])
def test_lidar_callsite_sequence_without_the_ground(cuda, harness, tmp_path, layout):
    frames, velo2img = cases.fuse_frames()
    g = spec.to_capi(cases.FUSE_GROUND)
    inp = tmp_path / "frames.bin"
    with open(inp, "wb") as f:
        f.write(struct.pack("<8i", scan_cases.FUSE_H, scan_cases.FUSE_W, len(frames), *scan_cases.FUSE_DIMS, FILL[0], FILL[1]))
        f.write(struct.pack("<2f", FILL[2], scan_cases.FUSE_VS))
        f.write(scan_cases.FUSE_ORIGIN.astype(F).tobytes())
        f.write(scan_cases.FUSE_K.astype(F).tobytes())
        f.write(np.ascontiguousarray(velo2img, F).tobytes())
        f.write(bytes(g))
        for c2w, pts, flags in frames:
            f.write(np.ascontiguousarray(c2w, F).tobytes())
            f.write(struct.pack("<i", len(pts)))
            f.write(pts.tobytes())
            f.write(cases.restated_depth(pts, flags, spec.DROP_GROUND, velo2img, FILL).tobytes())
    out = subprocess.run([harness, str(inp), layout], cwd=str(tmp_path), capture_output=True, text=True)
    assert out.returncode == 0 and "done" in out.stdout, out.stderr

    def files(i):
        return [(tmp_path / f"tsdf{i}.{ext}").read_bytes() for ext in ("bin", "ply")]

    # SetScanGround + SetScanFill + IntegrateScan == Integrate of the restated image, file for file
    assert files(1) == files(2)
    # ... set and then cleared == never set, and dropping the ground changed something
    assert files(5) == files(6)
    assert files(1)[0] != files(6)[0] and files(4)[0] != files(1)[0]
    # ... and every object's files are those of the same calls through capi.py
    with capi.Volume(config()) as v_drop_fill, capi.Volume(config()) as v_drop, capi.Volume(config()) as v_only, capi.Volume(config()) as v_fill:
        for c2w, pts, _ in frames:
            v_drop_fill.integrate_scan_ground(pts, velo2img, c2w, g, capi.SCAN_DROP_GROUND, fill_params=FILL)
            v_drop.integrate_scan_ground(pts, velo2img, c2w, g, capi.SCAN_DROP_GROUND)
            v_only.integrate_scan_ground(pts, velo2img, c2w, g, capi.SCAN_ONLY_GROUND, fill_params=FILL)
            v_fill.integrate_scan_filled(pts, velo2img, c2w, FILL)
        for i, vol in ((1, v_drop_fill), (3, v_drop), (4, v_only), (6, v_fill)):
            vol.save_bin(str(tmp_path / "want.bin"))
            vol.save_ply(str(tmp_path / "want.ply"))
            assert files(i) == [(tmp_path / "want.bin").read_bytes(), (tmp_path / "want.ply").read_bytes()], i
        _, w_all = v_fill.download()
        _, w_drop = v_drop_fill.download()
        assert np.count_nonzero(w_all) > np.count_nonzero(w_drop) > 1000
