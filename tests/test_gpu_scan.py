"""The lidar path on the device against its restatement (tests/scan_spec.py): projection of a scan, range to z-depth, and the
two fusing entry points.  The library builds with contraction off and correctly rounded division and square root, so every
comparison here is array_equal on the bit patterns: there is no tolerance anywhere.  The cases (tests/scan_cases.py) assert on
the CPU that the restatement reaches the branch each is named for."""
import ctypes as C

import numpy as np
import pytest

import scan_cases as cases
import scan_spec as spec
from semantic_slam_amd import capi, synth

pytestmark = pytest.mark.gpu

F = np.float32
TRUNC = float(F(cases.FUSE_VS) * F(5))


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def same(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def check_case(scanner, c):
    rng, dep, n = scanner.project(c["points"], c["velo2img"], c["K"])
    assert same(rng, c["range"]), c["name"]
    assert same(dep, c["depth"]), c["name"]
    assert n == c["n_pixels"], c["name"]


def test_every_small_case_through_one_scanner(cuda):
    """All cases of the 61 x 45 image through ONE scanner, one after the other: each sees a key image the one before it has
    left, so a scan that leaked into the next would show.  Then an empty scan: all-zero images."""
    small = cases.small_cases()
    with capi.Scanner(cases.H, cases.W) as sc:
        for c in small:
            check_case(sc, c)
        # outputs asked for one at a time: each alone equals what it was beside the others
        big = [c for c in small if c["name"] == "count_4097"][0]
        assert sc.project(big["points"], big["velo2img"], want_range=False, want_depth=False) == (None, None, big["n_pixels"])
        rng, dep, n = sc.project(big["points"], big["velo2img"], want_depth=False, want_count=False)
        assert same(rng, big["range"]) and dep is None and n is None
        rng, dep, n = sc.project(big["points"], big["velo2img"], big["K"], want_range=False, want_count=False)
        assert same(dep, big["depth"]) and rng is None
        # two different scans in a row, then an empty one
        check_case(sc, [c for c in small if c["name"] == "collide_1000_permuted"][0])
        check_case(sc, big)
        rng, dep, n = sc.project(np.zeros((0, 4), F), big["velo2img"], big["K"])
        assert n == 0 and not bits(rng).any() and not bits(dep).any()
        check_case(sc, [c for c in small if c["name"] == "count_65"][0])


def test_calibration_case(cuda):
    c = cases.calibration_case()
    with capi.Scanner(c["H"], c["W"]) as sc:
        check_case(sc, c)
        check_case(sc, c)


def test_composition_is_the_restatement(cuda):
    cal = cases.golden_calibration()
    got = capi.scan_projection(cal["P_rect"], cal["R_rect"], cal["R_velo"], cal["t_velo"])
    assert same(got, spec.compose(cal["P_rect"], cal["R_rect"], cal["R_velo"], cal["t_velo"]))


def test_range_to_depth_on_the_conversion_image(cuda):
    c = cases.conversion_case()
    with capi.Scanner(cases.H, cases.W) as sc:
        assert same(sc.range_to_depth(c["range"], c["K"]), c["depth"])
        big = [s for s in cases.small_cases() if s["name"] == "count_4097"][0]
        check_case(sc, big)                       # the conversion leaves the scanner's scans alone
        assert same(sc.range_to_depth(c["range"], c["K"]), c["depth"])


# ---- fusing -------------------------------------------------------------------------------------------------------
def fuse_config(z_begin=0, z_end=None, K=cases.FUSE_K):
    return capi.make_config(cases.FUSE_DIMS, cases.FUSE_VS, cases.FUSE_ORIGIN, K=K, z_begin=z_begin, z_end=z_end,
                            im_height=cases.FUSE_H, im_width=cases.FUSE_W)


def oracle_volume(oracle, depths, z_begin=0, z_end=None):
    """(tsdf, weight) of the oracle for the fuse frames' poses and the given depth images."""
    frames, _ = cases.fuse_frames()
    t, w = oracle.init_grid(cases.FUSE_DIMS, z_begin, z_end)
    changed = np.zeros(t.size, bool)
    for (c2w, _, _, _), depth in zip(frames, depths):
        before = w.copy()
        oracle.integrate(cases.FUSE_K, oracle.cam2base(synth.identity_pose(), c2w), depth, cases.FUSE_DIMS, cases.FUSE_ORIGIN,
                         cases.FUSE_VS, TRUNC, t, w, z_begin=z_begin, z_end=z_end)
        changed |= before != w
    return t, w, int(np.count_nonzero(changed))


@pytest.fixture(scope="module")
def scan_oracle(oracle):
    """The oracle's volume for the restated depth images of the three scans; not an empty comparison."""
    frames, _ = cases.fuse_frames()
    t, w, changed = oracle_volume(oracle, [f[3] for f in frames])
    assert changed >= 1000, changed
    return t, w


def assert_volume(vol, t, w, what):
    got_t, got_w = vol.download()
    assert np.array_equal(got_w, w), f"{what}: weights differ"
    assert np.array_equal(bits(got_t), bits(t)), f"{what}: TSDF differs"


@pytest.mark.parametrize("mode", ["deferral_off", "default", "interleaved"])
def test_integrate_scan_equals_integrate_of_the_restated_depth(cuda, scan_oracle, mode):
    frames, velo2img = cases.fuse_frames()
    big = [c for c in cases.small_cases() if c["name"] == "count_4097"][0]
    with capi.Volume(fuse_config()) as vol, capi.Volume(fuse_config()) as plain, capi.Scanner(cases.FUSE_H, cases.FUSE_W) as sc:
        if mode == "deferral_off":
            vol.set_deferral(0)
            plain.set_deferral(0)
        for c2w, pts, _, depth in frames:
            vol.integrate_scan(pts, velo2img, c2w)
            if mode == "interleaved":      # other scans through a scanner of the same size, between the handle's
                assert sc.project(pts[::3], velo2img, want_range=False, want_depth=False)[2] > 0
            plain.integrate(depth, c2w)
        assert_volume(vol, *scan_oracle, "integrate_scan")
        assert_volume(plain, *scan_oracle, "integrate of the restated depth")


@pytest.mark.parametrize("mode", ["deferral_off", "default"])
def test_integrate_range_of_a_masked_range_image(cuda, oracle, mode):
    """Engine.cpp:192-193 masks the image per instance: zeros outside the mask, ranges inside."""
    frames, _ = cases.fuse_frames()
    mask = np.zeros((cases.FUSE_H, cases.FUSE_W), bool)
    mask[9:61, 14:83] = True
    ranges = [np.where(mask, f[2], F(0)).astype(F) for f in frames]
    depths = [spec.range_to_depth(r, cases.FUSE_K) for r in ranges]
    t, w, changed = oracle_volume(oracle, depths)
    assert changed >= 1000 and all(np.count_nonzero(r) < np.count_nonzero(f[2]) for r, f in zip(ranges, frames))
    with capi.Volume(fuse_config()) as vol, capi.Volume(fuse_config()) as plain:
        if mode == "deferral_off":
            vol.set_deferral(0)
            plain.set_deferral(0)
        for (c2w, _, _, _), r, d in zip(frames, ranges, depths):
            vol.integrate_range(r, c2w)
            plain.integrate(d, c2w)
        assert_volume(vol, t, w, "integrate_range")
        assert_volume(plain, t, w, "integrate of the restated depth")


def test_integrate_scan_on_z_slabs(cuda, scan_oracle):
    frames, velo2img = cases.fuse_frames()
    dz = cases.FUSE_DIMS[2]
    per = cases.FUSE_DIMS[0] * cases.FUSE_DIMS[1]
    with capi.Volume(fuse_config(0, dz // 2)) as lo, capi.Volume(fuse_config(dz // 2, dz)) as hi, capi.Volume(fuse_config()) as whole:
        for c2w, pts, _, _ in frames:
            for v in (lo, hi, whole):
                v.integrate_scan(pts, velo2img, c2w)
        t, w = whole.download()
        assert_volume(whole, *scan_oracle, "whole grid")
        for v, a, b in ((lo, 0, dz // 2), (hi, dz // 2, dz)):
            assert_volume(v, t[a * per:b * per], w[a * per:b * per], f"slab [{a}, {b})")


def test_a_range_image_fused_as_depth_is_the_error_this_removes(cuda):
    frames, _ = cases.fuse_frames()
    with capi.Volume(fuse_config()) as as_range, capi.Volume(fuse_config()) as as_depth:
        for c2w, _, rng_im, _ in frames:
            as_range.integrate_range(rng_im, c2w)
            as_depth.integrate(rng_im, c2w)
        t_r, w_r = as_range.download()
        t_d, w_d = as_depth.download()
    assert w_r.sum() > 1000 and w_d.sum() > 1000
    assert np.count_nonzero(bits(t_r) != bits(t_d)) > 1000           # every surface fused too far away, off the axis


# ---- refusals -----------------------------------------------------------------------------------------------------
def refused(rc, lib, word):
    return rc == -1 and word.encode() in lib.tsdf_last_error()


def test_refusals(cuda):
    lib = capi.load()
    big = [c for c in cases.small_cases() if c["name"] == "count_65"][0]
    pts, m, k = big["points"], np.ascontiguousarray(big["velo2img"], F), np.ascontiguousarray(big["K"], F)
    img = np.zeros((cases.H, cases.W), F)
    n = C.c_int64()
    h = C.c_void_p()
    for hh, ww in ((0, 61), (45, 0), (-1, 61), (1 << 16, 1 << 15)):
        assert refused(lib.tsdf_scanner_create(0, hh, ww, C.byref(h)), lib, "image size")
    assert refused(lib.tsdf_scanner_create(0, 45, 61, None), lib, "NULL")
    assert refused(lib.tsdf_scanner_create(-1, 45, 61, C.byref(h)), lib, "device")
    assert refused(lib.tsdf_scan_projection(None, k.ctypes.data, k.ctypes.data, k.ctypes.data, m.ctypes.data), lib, "NULL")
    with capi.Scanner(cases.H, cases.W) as sc:
        s = sc._h
        P, K, R, D = pts.ctypes.data, k.ctypes.data, img.ctypes.data, img.ctypes.data
        assert refused(lib.tsdf_scan_project(None, m.ctypes.data, K, P, len(pts), R, D, C.byref(n)), lib, "NULL")
        assert refused(lib.tsdf_scan_project(s, None, K, P, len(pts), R, D, C.byref(n)), lib, "NULL")
        assert refused(lib.tsdf_scan_project(s, m.ctypes.data, K, None, len(pts), R, D, C.byref(n)), lib, "NULL")
        assert refused(lib.tsdf_scan_project(s, m.ctypes.data, None, P, len(pts), R, D, C.byref(n)), lib, "NULL")
        assert refused(lib.tsdf_scan_project(s, m.ctypes.data, K, P, len(pts), None, None, None), lib, "NULL")
        assert refused(lib.tsdf_scan_project(s, m.ctypes.data, K, P, -1, R, D, C.byref(n)), lib, "n_points")
        assert refused(lib.tsdf_scan_project(s, m.ctypes.data, K, P, 1 << 32, R, D, C.byref(n)), lib, "n_points")
        for bad in (np.nan, np.inf):
            mb = m.copy()
            mb[1, 2] = bad
            assert refused(lib.tsdf_scan_project(s, mb.ctypes.data, K, P, len(pts), R, D, C.byref(n)), lib, "velo2img")
            kb = k.copy()
            kb[2] = bad
            assert refused(lib.tsdf_scan_project(s, m.ctypes.data, kb.ctypes.data, P, len(pts), R, D, C.byref(n)), lib, "cam_K")
            assert refused(lib.tsdf_scan_range_to_depth(s, kb.ctypes.data, R, D), lib, "cam_K")
        for i in (0, 4):
            kb = k.copy()
            kb[i] = 0
            assert refused(lib.tsdf_scan_project(s, m.ctypes.data, kb.ctypes.data, P, len(pts), R, D, C.byref(n)), lib, "fx and fy")
            assert refused(lib.tsdf_scan_range_to_depth(s, kb.ctypes.data, R, D), lib, "fx and fy")
        assert refused(lib.tsdf_scan_range_to_depth(s, K, None, D), lib, "NULL")
        assert refused(lib.tsdf_scan_range_to_depth(s, K, R, None), lib, "NULL")
        # a non-finite cam_K is nobody's business while no depth is asked for
        kb = k.copy()
        kb[0] = np.nan
        assert lib.tsdf_scan_project(s, m.ctypes.data, kb.ctypes.data, P, len(pts), R, None, C.byref(n)) == 0
        assert n.value == big["n_pixels"] and same(img, big["range"])
        # the binding holds an image to the scanner's size
        with pytest.raises(ValueError):
            sc.range_to_depth(np.zeros((cases.H, cases.W + 1), F), k)
        with pytest.raises(ValueError):
            sc.project(np.zeros((5, 3), F), m)
        check_case(sc, big)                          # and after all of them the scanner works as before
    frames, velo2img = cases.fuse_frames()
    c2w, fpts, rng_im, _ = frames[0]
    pose = np.ascontiguousarray(c2w, F)
    vm = np.ascontiguousarray(velo2img, F)
    with capi.Volume(fuse_config()) as vol:
        v = vol._h
        assert refused(lib.tsdf_integrate_range(None, rng_im.ctypes.data, pose.ctypes.data), lib, "NULL")
        assert refused(lib.tsdf_integrate_range(v, None, pose.ctypes.data), lib, "NULL")
        assert refused(lib.tsdf_integrate_range(v, rng_im.ctypes.data, None), lib, "NULL")
        assert refused(lib.tsdf_integrate_scan(None, vm.ctypes.data, fpts.ctypes.data, len(fpts), pose.ctypes.data), lib, "NULL")
        assert refused(lib.tsdf_integrate_scan(v, None, fpts.ctypes.data, len(fpts), pose.ctypes.data), lib, "NULL")
        assert refused(lib.tsdf_integrate_scan(v, vm.ctypes.data, None, len(fpts), pose.ctypes.data), lib, "NULL")
        assert refused(lib.tsdf_integrate_scan(v, vm.ctypes.data, fpts.ctypes.data, len(fpts), None), lib, "NULL")
        assert refused(lib.tsdf_integrate_scan(v, vm.ctypes.data, fpts.ctypes.data, 1 << 32, pose.ctypes.data), lib, "n_points")
        mb = vm.copy()
        mb[0, 0] = np.inf
        assert refused(lib.tsdf_integrate_scan(v, mb.ctypes.data, fpts.ctypes.data, len(fpts), pose.ctypes.data), lib, "velo2img")
        t, w = vol.download()
        assert not w.any() and np.all(t == 1)           # nothing of the refused calls reached the volume
    for i, word in ((0, "fx and fy"), (4, "fx and fy"), (2, "cam_K")):
        kb = cases.FUSE_K.copy()
        kb[i] = 0 if i != 2 else np.nan
        with capi.Volume(fuse_config(K=kb)) as vol:
            assert refused(lib.tsdf_integrate_range(vol._h, rng_im.ctypes.data, pose.ctypes.data), lib, word)
            assert refused(lib.tsdf_integrate_scan(vol._h, vm.ctypes.data, fpts.ctypes.data, len(fpts), pose.ctypes.data), lib, word)


def test_empty_scan_fuses_nothing(cuda):
    frames, velo2img = cases.fuse_frames()
    with capi.Volume(fuse_config()) as vol:
        vol.integrate_scan(np.zeros((0, 4), F), velo2img, frames[0][0])
        t, w = vol.download()
    assert not w.any() and np.all(t == 1)
