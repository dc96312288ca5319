"""The lidar restatement (tests/scan_spec.py) on the CPU: every named case of tests/scan_cases.py reaches the branch it is named
for (the cases assert that as they are built), the serial semantics hold against a plain loop, and the known answers come out.
tests/test_gpu_scan.py holds the device to the same images."""
import numpy as np

import scan_cases as cases
import scan_spec as spec
from semantic_slam_amd import ingest, synth

F = np.float32


def serial_project(points, velo2img, H, W):
    """The reference's loop as it stands, one point after the other (ref: src/Utility.cpp:401-413 over :40-57)."""
    M = np.asarray(velo2img, F).reshape(3, 4)
    image = np.zeros((H, W), F)
    with np.errstate(all="ignore"):
        for x, y, z, _ in np.asarray(points, F).reshape(-1, 4):
            h = [F(F(F(F(M[k, 0] * x) + F(M[k, 1] * y)) + F(M[k, 2] * z)) + M[k, 3]) for k in range(3)]
            if not h[0] >= F(2):
                continue
            uf, vf = F(h[0] / h[2]), F(h[1] / h[2])
            if not (uf >= F(1) and uf < F(W) and vf >= F(1) and vf < F(H)):
                continue
            rng = np.sqrt(F(F(F(x * x) + F(y * y)) + F(z * z)))
            if rng > 0:
                image[int(vf), int(uf)] = rng
    return image


def test_every_small_case_reaches_its_branch_and_matches_the_serial_loop():
    names = [c["name"] for c in cases.small_cases()]
    assert len(names) == len(set(names)) and len(names) > 30
    for want in ("count_0", "count_1", "count_63", "count_64", "count_65", "count_4097", "collide_1000_in_order",
                 "collide_1000_permuted", "collide_64_and_4096_apart", "edge_h0_guard_a", "edge_uf_low_b", "edge_uf_high_a",
                 "edge_vf_low_a", "edge_vf_high_b", "edge_h2_zero_a", "edge_h2_negative_a", "edge_nan_x_a", "edge_inf_x_a",
                 "edge_zero_point_a", "edge_uf_beyond_int_a", "axis_point"):
        assert want in names, want
    for c in cases.small_cases():
        assert c["range"].shape == (cases.H, cases.W) and c["range"].dtype == F
        assert np.array_equal(serial_project(c["points"], c["velo2img"], cases.H, cases.W).view(np.uint32), c["range"].view(np.uint32)), c["name"]
        assert c["n_pixels"] == np.count_nonzero(c["range"])
        assert not c["range"][0].any() and not c["range"][:, 0].any()           # row 0 and column 0 are never written


def test_conversion_case():
    c = cases.conversion_case()
    r, K = c["range"], c["K"]
    # the rule per pixel, in scalars
    for v, u in ((0, 0), (1, 5), (1, 6), (22, 30), (44, 60), (13, 17)):
        x, y = F(F(F(u) - K[2]) / K[0]), F(F(F(v) - K[5]) / K[4])
        rim = np.sqrt(F(F(F(x * x) + F(y * y)) + F(1)))
        assert c["depth"][v, u].view(np.uint32) == F(r[v, u] / rim).view(np.uint32)


def test_calibration_case():
    c = cases.calibration_case()
    print(f"kitti calibration: {len(c['points'])} points, {c['n_pixels']} written pixels, "
          f"{np.count_nonzero(c['full']['reason'] == spec.ACCEPTED)} accepted")
    assert c["range"].shape == (375, 1242)
    d = c["depth"]
    assert np.count_nonzero(d) == c["n_pixels"] and np.all(d <= c["range"])


def test_composition_against_float64():
    cal = cases.golden_calibration()
    got = spec.compose(cal["P_rect"], cal["R_rect"], cal["R_velo"], cal["t_velo"])
    assert got.dtype == F and got.shape == (3, 4)
    P, A, B = np.zeros((4, 4)), np.eye(4), np.eye(4)
    P[:3] = cal["P_rect"]
    A[:3, :3] = cal["R_rect"]
    B[:3, :3], B[:3, 3] = cal["R_velo"], cal["t_velo"]
    want = (P @ A @ B)[:3]
    # two products of four-term float32 sums: each entry is off by at most a few roundings of the terms' magnitudes
    bound = 8 * np.finfo(F).eps * (np.abs(P) @ np.abs(A) @ np.abs(B))[:3]
    assert np.all(np.abs(got.astype(np.float64) - want) <= bound)
    assert abs(got[2, 0] - 1.0) < 1e-3 and abs(got[0, 1] + 707.0) < 5.0          # KITTI's: the camera looks along the sensor's x


def test_axis_point_known_answer():
    c = [c for c in cases.small_cases() if c["name"] == "axis_point"][0]
    assert c["range"][22, 30] == 2 and c["depth"][22, 30] == 2 and c["n_pixels"] == 1


def test_fuse_frames_give_the_oracle_something_to_fuse(oracle):
    frames, _ = cases.fuse_frames()
    t, w = oracle.init_grid(cases.FUSE_DIMS)
    trunc = float(F(cases.FUSE_VS) * F(5))
    for c2w, _, rng_im, depth in frames:
        assert np.count_nonzero(depth) == np.count_nonzero(rng_im) and np.any(depth < rng_im)
        oracle.integrate(cases.FUSE_K, c2w, depth, cases.FUSE_DIMS, cases.FUSE_ORIGIN, cases.FUSE_VS, trunc, t, w)
    assert np.count_nonzero(w) >= 1000


def test_synthetic_scan_is_a_kitti_file(tmp_path):
    scene = synth.SurfScene(cases.FUSE_DIMS, cases.FUSE_VS, cases.FUSE_ORIGIN, K=cases.FUSE_K, h=cases.FUSE_H, w=cases.FUSE_W)
    pts = synth.lidar_scan(scene, synth.identity_pose(), n_azimuth=360, elev_deg=(24.0, -24.0))
    assert pts.dtype == F and pts.ndim == 2 and pts.shape[1] == 4 and len(pts) > 500
    # every point lies on the scene: the sphere or the wall, seen from the sensor's mount
    p_cam = pts[:, :3].astype(np.float64) @ synth.VELO2CAM[:3, :3].T + synth.VELO2CAM[:3, 3]
    on_sphere = np.abs(np.linalg.norm(p_cam - scene.center, axis=1) - scene.radius) < 1e-5
    on_wall = np.abs(p_cam[:, 2] - scene.wall_z) < 1e-5
    assert np.all(on_sphere | on_wall) and on_sphere.any() and on_wall.any()
    path = tmp_path / "scan.bin"
    pts.tofile(path)
    assert np.array_equal(ingest.read_velodyne_bin(str(path)), pts)
    (tmp_path / "cut.bin").write_bytes(pts.tobytes()[:-4])
    try:
        ingest.read_velodyne_bin(str(tmp_path / "cut.bin"))
        raise AssertionError("a cut file must be refused")
    except ValueError:
        pass
