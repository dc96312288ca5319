"""The lidar gap fill on the device against its restatement (tests/scan_fill_spec.py): the fill alone, behind the projection,
and inside the two fusing entry points.  The library builds with contraction off, correctly rounded division and denormals
kept, so every comparison here is array_equal on the bit patterns: there is no tolerance anywhere.  The cases
(tests/scan_fill_cases.py) assert on the CPU that the restatement reaches the branch each is named for."""
import ctypes as C

import numpy as np
import pytest

import scan_cases
import scan_fill_cases as cases
import scan_fill_spec as spec
import scan_spec
from semantic_slam_amd import capi

pytestmark = pytest.mark.gpu

F = np.float32
FILL = (5, 8, 0.05)          # the default parameters: they add about 800 pixels to each of the fuse frames' 2 900


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def same(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def check_case(scanner, c):
    f, k, n = scanner.fill_depth(c["depth"], c["params"])
    assert same(f, c["filled"]), c["name"]
    assert np.array_equal(k, c["kind"]), c["name"]
    assert n == c["n_filled"], c["name"]


def by_shape(all_cases):
    out = {}
    for c in all_cases:
        out.setdefault((c["H"], c["W"]), []).append(c)
    return out


def test_default_parameters(cuda):
    p = capi.scan_fill_params_default()
    assert (p.max_span_u, p.max_span_v) == spec.DEFAULT[:2] and F(p.jump_rel) == spec.DEFAULT[2]


def test_every_small_case_through_one_scanner_per_shape(cuda):
    """All cases of a shape through ONE scanner, one after the other, then an empty image: nothing of a call stays behind."""
    for (h, w), group in by_shape(cases.small_cases()).items():
        with capi.Scanner(h, w) as sc:
            for c in group:
                check_case(sc, c)
            f, k, n = sc.fill_depth(np.zeros((h, w), F), (16, 16, 1e30))
            assert n == 0 and not bits(f).any() and not k.any()
            check_case(sc, group[0])
            # outputs asked for one at a time: each alone equals what it was beside the others
            c = group[-1]
            assert sc.fill_depth(c["depth"], c["params"], want_depth=False, want_kind=False) == (None, None, c["n_filled"])
            f, k, n = sc.fill_depth(c["depth"], c["params"], want_kind=False, want_count=False)
            assert same(f, c["filled"]) and k is None and n is None
            f, k, n = sc.fill_depth(c["depth"], c["params"], want_depth=False, want_count=False)
            assert f is None and np.array_equal(k, c["kind"]) and n is None


def test_in_place_host_buffers(cuda):
    for name in ("sparse_37x70_spans_5_8", "sparse_130x131_spans_16_16"):
        c = [c for c in cases.small_cases() if c["name"] == name][0]
        with capi.Scanner(c["H"], c["W"]) as sc:
            buf = c["depth"].copy()
            f, k, n = sc.fill_depth(buf, c["params"], in_place=True)
            assert f is buf and same(buf, c["filled"]) and np.array_equal(k, c["kind"]) and n == c["n_filled"]
            assert n > 0 and not same(c["depth"], c["filled"])


@pytest.mark.parametrize("seed", range(20))
def test_random_sparse_images(cuda, seed):
    c = cases.random_case(seed)
    with capi.Scanner(c["H"], c["W"]) as sc:
        check_case(sc, c)


def test_kitti_case(cuda):
    c = cases.kitti_case()
    s = scan_cases.calibration_case()
    with capi.Scanner(c["H"], c["W"]) as sc:
        check_case(sc, c)
        f, k, n = sc.project_filled(s["points"], s["velo2img"], s["K"])
        assert same(f, c["filled"]) and np.array_equal(k, c["kind"]) and n == c["n_filled"]
        check_case(sc, c)


def test_project_filled_on_the_fuse_frames(cuda):
    """tsdf_scan_project_filled against project -> range_to_depth -> fill, each through the restatement and through the device."""
    frames, velo2img = scan_cases.fuse_frames()
    with capi.Scanner(scan_cases.FUSE_H, scan_cases.FUSE_W) as sc:
        for _, pts, rng_im, depth in frames:
            want_f, want_k, want_n = spec.fill(depth, *FILL)
            assert want_n > 500
            f, k, n = sc.project_filled(pts, velo2img, scan_cases.FUSE_K, FILL)
            assert same(f, want_f) and np.array_equal(k, want_k) and n == want_n
            r, d, _ = sc.project(pts, velo2img, scan_cases.FUSE_K)
            assert same(r, rng_im) and same(d, depth)                                # the plain call is as it was
            f2, k2, n2 = sc.fill_depth(sc.range_to_depth(r, scan_cases.FUSE_K), FILL)
            assert same(f2, want_f) and np.array_equal(k2, want_k) and n2 == want_n
        f, k, n = sc.project_filled(np.zeros((0, 4), F), velo2img, scan_cases.FUSE_K, FILL)
        assert n == 0 and not bits(f).any() and not k.any()
        assert sc.project_filled(frames[0][1], velo2img, scan_cases.FUSE_K, FILL, want_depth=False, want_kind=False)[2] == \
            spec.fill(frames[0][3], *FILL)[2]


# ---- fusing -------------------------------------------------------------------------------------------------------
def fuse_config():
    return capi.make_config(scan_cases.FUSE_DIMS, scan_cases.FUSE_VS, scan_cases.FUSE_ORIGIN, K=scan_cases.FUSE_K,
                            im_height=scan_cases.FUSE_H, im_width=scan_cases.FUSE_W)


def band(t, w):
    return int(np.count_nonzero((w > 0) & (np.abs(t) < 1)))


def assert_same_volume(a, b, what):
    ta, wa = a.download()
    tb, wb = b.download()
    assert np.array_equal(wa, wb), f"{what}: weights differ"
    assert np.array_equal(bits(ta), bits(tb)), f"{what}: TSDF differs"
    return ta, wa


@pytest.mark.parametrize("deferral", [0, 4])
@pytest.mark.parametrize("call", ["scan", "range"])
def test_filled_integrate_equals_integrate_of_the_restated_filled_depth(cuda, deferral, call):
    frames, velo2img = scan_cases.fuse_frames()
    mask = np.zeros((scan_cases.FUSE_H, scan_cases.FUSE_W), bool)
    mask[9:61, 14:83] = True
    with capi.Volume(fuse_config()) as vol, capi.Volume(fuse_config()) as plain, capi.Volume(fuse_config()) as unfilled:
        for v in (vol, plain, unfilled):
            v.set_deferral(deferral)
        for c2w, pts, rng_im, depth in frames:
            if call == "scan":
                vol.integrate_scan_filled(pts, velo2img, c2w, FILL)
                unfilled.integrate_scan(pts, velo2img, c2w)
                sparse = depth
            else:                                                        # a masked range image, as the reference's object loop makes
                masked = np.where(mask, rng_im, F(0)).astype(F)
                vol.integrate_range_filled(masked, c2w, FILL)
                unfilled.integrate_range(masked, c2w)
                sparse = scan_spec.range_to_depth(masked, scan_cases.FUSE_K)
            want, _, n = spec.fill(sparse, *FILL)
            assert n > 300
            plain.integrate(want, c2w)
        t, w = assert_same_volume(vol, plain, f"integrate_{call}_filled")
        tu, wu = unfilled.download()
        assert band(t, w) > band(tu, wu) > 100


def test_filled_calls_interleaved_with_plain_ones(cuda):
    """Filled and unfilled calls in turn on one handle, deferral on: each frame is what its own call makes of it."""
    frames, velo2img = scan_cases.fuse_frames()
    with capi.Volume(fuse_config()) as vol, capi.Volume(fuse_config()) as plain:
        vol.set_deferral(4)
        plain.set_deferral(4)
        for rounds in range(2):
            for i, (c2w, pts, rng_im, depth) in enumerate(frames):
                filled = spec.fill(depth, *FILL)[0]
                if i % 2 == 0:
                    vol.integrate_scan_filled(pts, velo2img, c2w, FILL)
                    vol.integrate_scan(pts, velo2img, c2w)
                else:
                    vol.integrate_range_filled(rng_im, c2w, FILL)
                    vol.integrate_range(rng_im, c2w)
                plain.integrate(filled, c2w)
                plain.integrate(depth, c2w)
        assert_same_volume(vol, plain, "interleaved")


# ---- refusals -----------------------------------------------------------------------------------------------------
def refused(rc, lib, word):
    return rc == -1 and word.encode() in lib.tsdf_last_error()


def test_refusals(cuda):
    lib = capi.load()
    c = [c for c in cases.small_cases() if c["name"] == "sparse_37x70_spans_5_8"][0]
    frames, velo2img = scan_cases.fuse_frames()
    c2w, pts, rng_im, _ = frames[0]
    good = capi.ScanFillParams(5, 8, 0.05)
    bad = [capi.ScanFillParams(-1, 8, 0.05), capi.ScanFillParams(5, 17, 0.05), capi.ScanFillParams(17, 8, 0.05),
           capi.ScanFillParams(5, -1, 0.05)]
    bad_jump = [capi.ScanFillParams(5, 8, -0.01), capi.ScanFillParams(5, 8, float("nan")), capi.ScanFillParams(5, 8, float("inf"))]
    out = np.zeros((c["H"], c["W"]), F)
    kind = np.zeros((c["H"], c["W"]), np.uint8)
    n = C.c_int64()
    assert refused(lib.tsdf_scan_fill_params_default(None), lib, "NULL")
    with capi.Scanner(c["H"], c["W"]) as sc:
        s, D, O, Kd = sc._h, c["depth"].ctypes.data, out.ctypes.data, kind.ctypes.data
        assert refused(lib.tsdf_scan_fill_depth(None, C.addressof(good), D, O, Kd, C.byref(n)), lib, "NULL")
        assert refused(lib.tsdf_scan_fill_depth(s, None, D, O, Kd, C.byref(n)), lib, "NULL")
        assert refused(lib.tsdf_scan_fill_depth(s, C.addressof(good), None, O, Kd, C.byref(n)), lib, "NULL")
        assert refused(lib.tsdf_scan_fill_depth(s, C.addressof(good), D, None, None, None), lib, "NULL")
        for p in bad:
            assert refused(lib.tsdf_scan_fill_depth(s, C.addressof(p), D, O, Kd, C.byref(n)), lib, "max_span")
        for p in bad_jump:
            assert refused(lib.tsdf_scan_fill_depth(s, C.addressof(p), D, O, Kd, C.byref(n)), lib, "jump_rel")
        with pytest.raises(ValueError):
            sc.fill_depth(np.zeros((c["H"], c["W"] + 1), F))
        check_case(sc, c)                              # and after all of them the scanner works as before
    m, k = np.ascontiguousarray(velo2img, F), np.ascontiguousarray(scan_cases.FUSE_K, F)
    pose = np.ascontiguousarray(c2w, F)
    out = np.zeros((scan_cases.FUSE_H, scan_cases.FUSE_W), F)
    with capi.Scanner(scan_cases.FUSE_H, scan_cases.FUSE_W) as sc:
        s, M, K, P, G, O = sc._h, m.ctypes.data, k.ctypes.data, pts.ctypes.data, C.addressof(good), out.ctypes.data
        assert refused(lib.tsdf_scan_project_filled(None, M, K, G, P, len(pts), O, None, None), lib, "NULL")
        assert refused(lib.tsdf_scan_project_filled(s, None, K, G, P, len(pts), O, None, None), lib, "NULL")
        assert refused(lib.tsdf_scan_project_filled(s, M, None, G, P, len(pts), O, None, None), lib, "NULL")
        assert refused(lib.tsdf_scan_project_filled(s, M, K, None, P, len(pts), O, None, None), lib, "NULL")
        assert refused(lib.tsdf_scan_project_filled(s, M, K, G, None, len(pts), O, None, None), lib, "NULL")
        assert refused(lib.tsdf_scan_project_filled(s, M, K, G, P, len(pts), None, None, None), lib, "NULL")
        assert refused(lib.tsdf_scan_project_filled(s, M, K, G, P, -1, O, None, None), lib, "n_points")
        assert refused(lib.tsdf_scan_project_filled(s, M, K, C.addressof(bad[1]), P, len(pts), O, None, None), lib, "max_span")
        assert refused(lib.tsdf_scan_project_filled(s, M, K, C.addressof(bad_jump[1]), P, len(pts), O, None, None), lib, "jump_rel")
        kb = k.copy()
        kb[0] = 0
        assert refused(lib.tsdf_scan_project_filled(s, M, kb.ctypes.data, G, P, len(pts), O, None, None), lib, "fx and fy")
    with capi.Volume(fuse_config()) as vol:
        v, R = vol._h, rng_im.ctypes.data
        assert refused(lib.tsdf_integrate_range_filled(None, G, R, pose.ctypes.data), lib, "NULL")
        assert refused(lib.tsdf_integrate_range_filled(v, None, R, pose.ctypes.data), lib, "NULL")
        assert refused(lib.tsdf_integrate_range_filled(v, G, None, pose.ctypes.data), lib, "NULL")
        assert refused(lib.tsdf_integrate_range_filled(v, G, R, None), lib, "NULL")
        assert refused(lib.tsdf_integrate_range_filled(v, C.addressof(bad[0]), R, pose.ctypes.data), lib, "max_span")
        assert refused(lib.tsdf_integrate_scan_filled(None, M, G, P, len(pts), pose.ctypes.data), lib, "NULL")
        assert refused(lib.tsdf_integrate_scan_filled(v, None, G, P, len(pts), pose.ctypes.data), lib, "NULL")
        assert refused(lib.tsdf_integrate_scan_filled(v, M, None, P, len(pts), pose.ctypes.data), lib, "NULL")
        assert refused(lib.tsdf_integrate_scan_filled(v, M, G, None, len(pts), pose.ctypes.data), lib, "NULL")
        assert refused(lib.tsdf_integrate_scan_filled(v, M, G, P, len(pts), None), lib, "NULL")
        assert refused(lib.tsdf_integrate_scan_filled(v, M, C.addressof(bad_jump[0]), P, len(pts), pose.ctypes.data), lib, "jump_rel")
        t, w = vol.download()
        assert not w.any() and np.all(t == 1)           # nothing of the refused calls reached the volume
