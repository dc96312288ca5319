"""The extent rule (csrc/tsdf_extent.hip.h) in its restatement tests/extent_spec.py, and the host-only calls of the C ABI
(tsdf_extent_params_default / _combine / _metric / _regrid) through the loaded library, without a GPU: known answers on
hand-made volumes, the classification of the value edges, slab records that combine to the whole grid's, the metric form
against double arithmetic, the proposed grid's exact dims and origin bits, every refusal, and that the parity cases of
tests/test_gpu_extent.py are not vacuous."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import extent_cases as ec
import extent_spec as es
from semantic_slam_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32


def fresh(dims):
    n = int(np.prod(dims))
    return np.ones(n, f32), np.zeros(n, f32)


def flat(dims, x, y, z):
    return (z * dims[1] + y) * dims[0] + x


# ------------------------------------------------------------------------------------------------------------------------
# the restatement on volumes with known answers
# ------------------------------------------------------------------------------------------------------------------------
def test_empty_grid():
    dims = (7, 5, 3)
    rec = es.extent(*fresh(dims), dims, margin=2)
    assert rec == es.empty(dims)
    assert rec["lo"] == [7, 5, 3] and rec["hi"] == [-1, -1, -1] and rec["n_observed"] == 0


def test_single_voxel():
    dims = (7, 5, 3)
    t, w = fresh(dims)
    i = flat(dims, 5, 1, 2)
    t[i], w[i] = 0.25, 2.0
    t[flat(dims, 0, 0, 0)], w[flat(dims, 0, 0, 0)] = 1.0, 3.0      # observed free space: counted as observed only
    rec = es.extent(t, w, dims, margin=2)
    assert rec == {"n_observed": 2, "n_surface": 1, "sum": [5, 1, 2], "sum2": [25, 1, 4, 5, 10, 2],
                   "border": [0, 1, 1, 0, 0, 1], "lo": [5, 1, 2], "hi": [5, 1, 2]}
    assert es.extent(t, w, dims, margin=0)["border"] == [0] * 6
    assert es.extent(t, w, dims, margin=9)["border"] == [1] * 6     # a margin beyond the dims: near every face


def test_filled_box():
    dims = (9, 8, 6)
    t, w = fresh(dims)
    t3, w3 = t.reshape(dims[::-1]), w.reshape(dims[::-1])
    (x0, x1), (y0, y1), (z0, z1) = (2, 6), (0, 4), (3, 5)           # inclusive
    t3[z0:z1 + 1, y0:y1 + 1, x0:x1 + 1], w3[z0:z1 + 1, y0:y1 + 1, x0:x1 + 1] = -0.5, 1.0
    rec = es.extent(t, w, dims, margin=1)
    nx, ny, nz = 5, 5, 3
    s1 = lambda a, b: sum(range(a, b + 1))
    s2 = lambda a, b: sum(v * v for v in range(a, b + 1))
    assert rec["n_surface"] == rec["n_observed"] == nx * ny * nz
    assert rec["sum"] == [s1(x0, x1) * ny * nz, s1(y0, y1) * nx * nz, s1(z0, z1) * nx * ny]
    assert rec["sum2"] == [s2(x0, x1) * ny * nz, s2(y0, y1) * nx * nz, s2(z0, z1) * nx * ny,
                           s1(x0, x1) * s1(y0, y1) * nz, s1(x0, x1) * s1(z0, z1) * ny, s1(y0, y1) * s1(z0, z1) * nx]
    assert rec["border"] == [0, 0, nx * nz, 0, 0, nx * ny]           # the box touches y- and z+
    assert rec["lo"] == [x0, y0, z0] and rec["hi"] == [x1, y1, z1]


def test_edge_values_are_classified_as_the_rule_says():
    one_below = np.nextafter(f32(1), f32(0))
    above = np.nextafter(f32(0.9), f32(1))
    # in the order of extent_cases.EDGE_T: +0, -0, 1, -1, the floats next to +-1 inside the band, NaN, +inf, -inf
    surface_at_band_1 = [True, True, False, False, True, True, False, False, False]
    want_t = np.array([0.0, -0.0, 1.0, -1.0, one_below, -one_below, np.nan, np.inf, -np.inf], f32)
    assert np.array_equal(ec.EDGE_T.view(np.uint32), want_t.view(np.uint32))
    assert np.array_equal(ec.EDGE_W.view(np.uint32), np.array([0.9, above, np.nan], f32).view(np.uint32))
    for tv, near in zip(ec.EDGE_T, surface_at_band_1):
        for wv, observed in zip(ec.EDGE_W, (False, True, False)):
            obs, surf = es.classify([tv], [wv], 0.9, 1.0)
            assert bool(obs[0]) == observed, (tv, wv)
            assert bool(surf[0]) == (observed and near), (tv, wv)
    # a band below 1: the bound is strict there as well
    obs, surf = es.classify([0.25, np.nextafter(f32(0.25), f32(0)), -0.25], [1.0, 1.0, 1.0], 0.9, 0.25)
    assert obs.tolist() == [True, True, True] and surf.tolist() == [False, True, False]


# ------------------------------------------------------------------------------------------------------------------------
# the host-only calls of the library
# ------------------------------------------------------------------------------------------------------------------------
def test_struct_layouts_match_c(tmp_path):
    mirrors = {"tsdf_extent_params": capi.ExtentParams, "tsdf_extent": capi.Extent, "struct tsdf_extent_metric": capi.ExtentMetric}
    body = ""
    for name, cls in mirrors.items():
        body += f'printf("{name.split()[-1]} size %zu\\n", sizeof({name}));\n'
        body += "".join(f'printf("{name.split()[-1]} {f} %zu\\n", offsetof({name}, {f}));\n' for f, _ in cls._fields_)
    prog = tmp_path / "layout.c"
    prog.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "tsdf_hip.h"\nint main(void){\n' + body + "return 0;}\n")
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(prog), "-o", str(exe)])
    got = {tuple(line.split()[:2]): int(line.split()[2]) for line in subprocess.check_output([str(exe)]).decode().splitlines()}
    for name, cls in mirrors.items():
        name = name.split()[-1]
        assert got[(name, "size")] == C.sizeof(cls), name
        for f, _ in cls._fields_:
            assert got[(name, f)] == getattr(cls, f).offset, (name, f)


def test_params_default():
    p = capi.extent_params_default(capi.default_config())               # the reference's grid: 4 mm voxels, band 5 voxels
    assert f32(p.weight_thresh) == f32(0.9) and p.band == 1.0 and p.margin == 5
    cfg = capi.make_config((8, 8, 8), 0.004, np.zeros(3, f32), trunc=0.0101)
    assert capi.extent_params_default(cfg).margin == 3                  # ceil(2.525)
    lib = capi.load()
    assert lib.tsdf_extent_params_default(None, C.byref(p)) == -1 and b"NULL" in lib.tsdf_last_error()
    assert lib.tsdf_extent_params_default(C.byref(cfg), None) == -1 and b"NULL" in lib.tsdf_last_error()


@pytest.mark.parametrize("state", ["random", "edges"])
def test_combine_of_slab_records_is_the_whole_grids(state):
    dims = (20, 12, 9)
    t, w = ec.state(dims, state)
    slice_n = dims[0] * dims[1]
    for margin in ec.margins(dims):
        whole = es.extent(t, w, dims, margin=margin)
        assert whole["n_surface"] > 0
        for cut in range(0, dims[2] + 1):                               # every z, the empty slabs at both ends included
            lo = es.extent(t[:cut * slice_n], w[:cut * slice_n], dims, 0, cut, margin=margin)
            hi = es.extent(t[cut * slice_n:], w[cut * slice_n:], dims, cut, dims[2], margin=margin)
            assert es.combine(lo, hi) == whole
            got = capi.extent_combine(capi.Extent.from_dict(lo), capi.Extent.from_dict(hi))
            assert got.as_dict() == whole, (margin, cut)
    three = [es.extent(t[a * slice_n:b * slice_n], w[a * slice_n:b * slice_n], dims, a, b, margin=1) for a, b in ((0, 3), (3, 7), (7, 9))]
    acc = capi.Extent.from_dict(three[0])
    for part in three[1:]:
        acc = capi.extent_combine(acc, capi.Extent.from_dict(part))
    assert acc.as_dict() == es.extent(t, w, dims, margin=1)
    lib = capi.load()
    e = capi.Extent()
    for args in ((None, C.byref(e), C.byref(e)), (C.byref(e), None, C.byref(e)), (C.byref(e), C.byref(e), None)):
        assert lib.tsdf_extent_combine(*args) == -1 and b"tsdf_extent_combine" in lib.tsdf_last_error()


def test_metric_against_double_arithmetic():
    dims = (72, 33, 17)
    t, w = ec.state(dims, "fused")
    rec = es.extent(t, w, dims, band=0.25, margin=1)
    from semantic_slam_amd import synth
    b2w = synth.make_pose(synth.rot_z(0.3) @ synth.rot_x(-0.2), [0.4, -0.1, 2.0])
    cfg = capi.make_config(dims, 0.004, ec.origin_of(dims), base2world=b2w)
    got = capi.extent_metric(cfg, capi.Extent.from_dict(rec))
    want = es.metric(rec, ec.origin_of(dims), 0.004, b2w)
    for name in want:
        assert np.allclose(got[name], want[name], rtol=1e-12, atol=0.0), (name, got[name], want[name])
    # the same numbers from the voxels themselves (float64 NumPy over the surface voxels' coordinates)
    _, surf = es.classify(t, w, 0.9, 0.25)
    zi, yi, xi = np.nonzero(surf.reshape(dims[::-1]))
    pts = ec.origin_of(dims).astype(np.float64) + np.stack([xi, yi, zi], 1) * float(f32(0.004))
    assert np.allclose(got["centroid_base"], pts.mean(0), rtol=1e-9)
    cov = np.cov(pts.T, bias=True)
    assert np.allclose(got["cov_base"], [cov[i, j] for i, j in es.PAIRS], rtol=1e-6, atol=1e-12)
    B = np.asarray(b2w, np.float64).reshape(4, 4)
    assert np.allclose(got["centroid_world"], B[:3, :3] @ got["centroid_base"] + B[:3, 3], rtol=1e-12)
    assert np.all(got["lo_base"] < pts.min(0)) and np.all(got["hi_base"] > pts.max(0))
    lib = capi.load()
    m = capi.ExtentMetric()
    none = capi.Extent.from_dict(es.empty(dims))
    assert lib.tsdf_extent_metric(C.byref(cfg), C.byref(none), C.byref(m)) == -1 and b"n_surface" in lib.tsdf_last_error()
    e = capi.Extent.from_dict(rec)
    for args in ((None, C.byref(e), C.byref(m)), (C.byref(cfg), None, C.byref(m)), (C.byref(cfg), C.byref(e), None)):
        assert lib.tsdf_extent_metric(*args) == -1 and b"NULL" in lib.tsdf_last_error()


def test_regrid_dims_origin_bits_and_refusals():
    dims = (24, 18, 10)
    origin = np.array([-0.0471, 0.0312, 0.9017], f32)                   # no multiples of the voxel size: the roundings show
    cfg = capi.make_config(dims, 0.004, origin, z_begin=2, z_end=7)
    rec = es.empty(dims)
    rec.update(n_surface=5, lo=[3, 0, 2], hi=[23, 11, 9])
    e = capi.Extent.from_dict(rec)
    for pad, mult in ((0, 1), (5, 4), (2, 7), (40, 4)):                  # pad 5 and 40: indices below 0, the grid grows outward
        out = capi.extent_regrid(cfg, e, pad, mult)
        want_dims, want_origin = es.regrid(rec, origin, 0.004, pad, mult)
        assert (out.dim_x, out.dim_y, out.dim_z) == want_dims, (pad, mult)
        assert all(d % mult == 0 and d >= h - l + 1 + 2 * pad for d, l, h in zip(want_dims, rec["lo"], rec["hi"]))
        assert np.array_equal(np.array(out.origin, f32).view(np.uint32), want_origin.view(np.uint32)), (pad, mult)
        assert (out.z_begin, out.z_end) == (0, out.dim_z)
        assert (out.voxel_size, out.trunc_margin, out.im_height, list(out.cam_K), list(out.base2world)) == \
               (cfg.voxel_size, cfg.trunc_margin, cfg.im_height, list(cfg.cam_K), list(cfg.base2world))
    assert es.regrid(rec, origin, 0.004, 5, 4)[0] == (32, 24, 20)
    lib = capi.load()
    out = capi.TsdfConfig()

    def refused(cfg_, e_, pad, mult, word, out_=out):
        rc = lib.tsdf_extent_regrid(C.byref(cfg_) if cfg_ is not None else None, C.byref(e_) if e_ is not None else None, pad, mult,
                                    C.byref(out_) if out_ is not None else None)
        msg = lib.tsdf_last_error().decode()
        assert rc == -1 and "tsdf_extent_regrid" in msg and word in msg, (rc, msg, word)

    refused(None, e, 1, 4, "NULL")
    refused(cfg, None, 1, 4, "NULL")
    refused(cfg, e, 1, 4, "NULL", out_=None)
    refused(cfg, capi.Extent.from_dict(es.empty(dims)), 1, 4, "n_surface")
    refused(cfg, e, -1, 4, "pad_voxels")
    refused(cfg, e, 1, 0, "dim_multiple")
    huge = dict(rec, hi=[23, 70000 * 4, 9])                              # dim_y beyond what tsdf_create launches
    refused(cfg, capi.Extent.from_dict(huge), 0, 1, "launch limits")
    huge = dict(rec, hi=[(1 << 20), (1 << 12), 9])                       # a slice of more than 2^31 voxels
    refused(cfg, capi.Extent.from_dict(huge), 0, 1, "slice")
    refused(cfg, e, 0x7fffffff, 1, "32 bits")
    bad = capi.make_config(dims, 0.004, origin)
    bad.voxel_size = 0.0
    refused(bad, e, 1, 4, "voxel_size")


# ------------------------------------------------------------------------------------------------------------------------
# the GPU parity cases, through the restatement alone
# ------------------------------------------------------------------------------------------------------------------------
def test_the_gpu_parity_cases_are_not_vacuous():
    """Every case of tests/test_gpu_extent.py's parity test has at least 10 % of its voxels near a surface and at least 1 %
    observed but not near one.  With margin 1 all six border counts are above 0 in every case of the random and the
    edge-valued states (whose surface voxels reach every face, so their lo is 0); that the bounds are not always the grid's
    own is shown by the fused states, one of which at least has lo > 0 on some axis -- the two conditions exclude each other
    within one case.  margin 0 counts nothing; the largest margin counts every surface voxel for both faces of the
    shortest axis."""
    lo_above_zero = 0
    for dims in ec.SHAPES:
        n = int(np.prod(dims))
        for name in ec.states_of(dims):
            t, w = ec.state(dims, name)
            for band in ec.BANDS:
                recs = {m: es.extent(t, w, dims, band=band, margin=m) for m in ec.margins(dims)}
                rec = recs[1]
                assert rec["n_surface"] >= 0.10 * n, (dims, name, band, rec["n_surface"] / n)
                assert rec["n_observed"] - rec["n_surface"] >= 0.01 * n, (dims, name, band)
                if name != "fused":
                    assert min(rec["border"]) > 0, (dims, name, band, rec["border"])
                lo_above_zero += any(v > 0 for v in rec["lo"])
                assert recs[0]["border"] == [0] * 6
                axis = int(np.argmin(dims))
                big = recs[ec.margins(dims)[2]]
                assert big["border"][2 * axis] == big["border"][2 * axis + 1] == rec["n_surface"]
    assert lo_above_zero >= 1
    # the shapes whose slices take more than one workgroup have uploaded states only; one of them has 33 tiles, one rows that
    # are no multiple of 4 voxels, one an x whose square does not fit 32 bits
    wide = [d for d in ec.SHAPES if ec.workgroups_per_slice(d) > 1]
    assert all(ec.states_of(d) == ["random", "edges"] for d in wide) and len(wide) == 3
    assert (96, 88, 3) in wide and any(d[0] % 4 for d in wide)
    assert any(es.extent(*ec.state(d, "random"), d)["hi"][0] ** 2 >= 2 ** 32 for d in wide)
    t, w = ec.state((20, 12, 9), "edges")                               # the edge state holds every pair of the two lists
    for tv in ec.EDGE_T:
        for wv in ec.EDGE_W:
            same_t = np.isnan(t) if np.isnan(tv) else (t == tv) & (np.signbit(t) == np.signbit(tv))
            same_w = np.isnan(w) if np.isnan(wv) else w == wv
            assert (same_t & same_w).any(), (tv, wv)
