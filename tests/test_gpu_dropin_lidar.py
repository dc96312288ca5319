"""Drop-in proof for the second sensor: a C++ program written against include/tsdf.hpp as the reference's lidar labeller drives
its TSDF member (tests/dropin_lidar.cpp: scan -> range image -> instance mask -> the object's volume) writes, through
IntegrateRange and IntegrateScan, the files a TSDF fed the restated z-depth writes -- byte for byte, on one device and with
the grid cut into two z-slabs."""
import os
import struct
import subprocess

import numpy as np
import pytest

import scan_cases as cases
import scan_spec as spec
from semantic_slam_amd import synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "semantic_slam_amd")
F = np.float32


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("dropin_lidar") / "dropin_lidar")
    subprocess.check_call(["g++", "-O1", "-std=c++11", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "dropin_lidar.cpp"), "-o", exe,
                           "-L", PKG, "-ltsdf_dropin", "-ltsdf_hip", f"-Wl,-rpath,{PKG}"])
    return exe


@pytest.mark.parametrize("layout", ["single", "slabs"])
def test_lidar_callsite_sequence(cuda, oracle, harness, tmp_path, layout):
    frames, velo2img = cases.fuse_frames()
    mask = np.zeros((cases.FUSE_H, cases.FUSE_W), np.uint8)
    mask[9:61, 14:83] = 255
    inp = tmp_path / "frames.bin"
    masked_depths = []
    with open(inp, "wb") as f:
        f.write(struct.pack("<6i", cases.FUSE_H, cases.FUSE_W, len(frames), *cases.FUSE_DIMS))
        f.write(struct.pack("<f", cases.FUSE_VS))
        f.write(cases.FUSE_ORIGIN.astype(F).tobytes())
        f.write(cases.FUSE_K.astype(F).tobytes())
        f.write(np.ascontiguousarray(velo2img, F).tobytes())
        for c2w, pts, rng_im, _ in frames:
            restated = spec.range_to_depth(np.where(mask == 255, rng_im, F(0)).astype(F), cases.FUSE_K)
            masked_depths.append(restated)
            f.write(np.ascontiguousarray(c2w, F).tobytes())
            f.write(struct.pack("<i", len(pts)))
            f.write(pts.tobytes())
            f.write(mask.tobytes())
            f.write(restated.tobytes())
    out = subprocess.run([harness, str(inp), layout], cwd=str(tmp_path), capture_output=True, text=True)
    assert out.returncode == 0 and "done" in out.stdout, out.stderr
    # IntegrateRange of the masked ranges == Integrate of their restated depth, file for file
    for ext in ("bin", "ply"):
        assert (tmp_path / f"tsdf1.{ext}").read_bytes() == (tmp_path / f"tsdf2.{ext}").read_bytes(), ext
    # ... and both, and IntegrateScan's, are the oracle's files for the restated depth images
    trunc = float(F(cases.FUSE_VS) * F(5))
    updated = {}
    for vol_id, depths in ((1, masked_depths), (3, [fr[3] for fr in frames])):
        t, w = oracle.init_grid(cases.FUSE_DIMS)
        for (c2w, _, _, _), d in zip(frames, depths):
            oracle.integrate(cases.FUSE_K, oracle.cam2base(synth.identity_pose(), c2w), d, cases.FUSE_DIMS, cases.FUSE_ORIGIN,
                             cases.FUSE_VS, trunc, t, w)
        updated[vol_id] = np.count_nonzero(w)
        assert updated[vol_id] > 1000
        oracle.save_bin(str(tmp_path / "want.bin"), t, cases.FUSE_DIMS, cases.FUSE_ORIGIN, cases.FUSE_VS, trunc)
        oracle.save_ply(str(tmp_path / "want.ply"), t, w, cases.FUSE_DIMS, cases.FUSE_VS, cases.FUSE_ORIGIN)
        assert (tmp_path / f"tsdf{vol_id}.bin").read_bytes() == (tmp_path / "want.bin").read_bytes(), vol_id
        assert (tmp_path / f"tsdf{vol_id}.ply").read_bytes() == (tmp_path / "want.ply").read_bytes(), vol_id
    assert updated[1] < updated[3]               # the mask took something away
