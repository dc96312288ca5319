"""The photometric tracking rule (csrc/tsdf_photo.hip.h, restated in tests/photo_spec.py) means what it says, on the CPU:

  * without an rgb image or with photo_weight 0 the restatement's track is track_spec.track's, field for field;
  * J has the rule's sign and convention: its prediction of the residuals' change under a small step matches the change
    itself, and one combined step from a perturbed pose lowers the photometric cost on every convergence case;
  * every named case of tests/photo_cases.py reaches the branch it is named for;
  * facing a textured wall from a guess shifted in the plane, the depth-only track stays where it started and the combined
    track ends within one voxel edge of the truth;
  * tsdf_photo_params_default and the two new struct layouts (host only, no GPU).

The volumes are fused by photo_cases.cpu_fuse and rendered by raycast_spec; test_gpu_track_rgbd.py holds the device to the
same restatement over the device's own volumes and renders."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import photo_cases as pc
import photo_spec as ps
import raycast_spec as rs
import track_cases as tc
import track_spec as ts
from test_gpu_raycast import edge_state
from semantic_slam_amd import capi

f32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EYE34 = np.hstack([np.eye(3), np.zeros((3, 1))])


@pytest.fixture(scope="module")
def world():
    states = {k: pc.cpu_fuse(k) for k in ("scene", "wall")}
    n = int(np.prod(pc.DIMS))
    states["edge"] = edge_state(pc.DIMS, np.random.default_rng(tc.EDGE_SEED)) + (pc.edge_colours(n, np.random.default_rng(52)),)
    trunc = float(f32(pc.VS) * f32(5))

    def render(volume, ray, pose):
        hw = (ray.im_height, ray.im_width)
        t, w, _ = states[volume]
        o = rs.render(t, w, pc.DIMS, pc.origin_of(), pc.VS, trunc, np.asarray(ray.cam_K, f32), hw, ray.near_m, ray.far_m,
                      ray.weight_thresh, pose)
        return o["depth"].reshape(hw), o["normal"].reshape(hw + (3,))

    return pc.PhotoWorld(states, render)


# ------------------------------------------------------------------------------------------------------------------------
# the pieces
# ------------------------------------------------------------------------------------------------------------------------
def test_luminance_and_pyramid():
    assert ps.luma(0, 0, 0) == 0.0 and ps.luma(255, 255, 255) <= 1.0 and ps.luma(255, 255, 255) > 0.9999
    assert ps.luma_packed(np.uint32(0x00112233)) == ps.luma(0x33, 0x22, 0x11)        # 0x00BBGGRR
    I = np.arange(35, dtype=f32).reshape(5, 7) / 64
    I[2, 3] = -1
    h = ps.halve(I)
    assert h.shape == (2, 3)
    assert h[0, 0] == ((I[0, 0] + I[0, 1]) + (I[1, 0] + I[1, 1])) * f32(0.25)
    assert h[1, 1] == -1 and (np.delete(h.ravel(), 4) >= 0).all()                     # one invalid child invalidates the parent
    assert [p.shape for p in ps.pyramid(np.zeros((97, 161), f32))] == [(97, 161), (48, 80), (24, 40)]
    assert [p.shape for p in ps.pyramid(np.zeros((1, 3), f32))] == [(1, 3), (0, 1), (0, 0)]


def test_without_colour_it_is_the_geometric_track(world):
    for c in pc.convergence_cases()[:2] + pc.state_cases()[1:]:
        model = world.model(c)
        want = ts.track((c.live, c.mask), model[:2], c.P())
        for live, PP in (((c.live, c.mask, None), c.PP()), (c.live_tuple(), ps.photo_params(0.0))):
            got = ps.track(live, model, c.P(), PP)
            assert got["photo_pairs"] == 0
            for k, v in want.items():
                assert np.array_equal(got[k], v), (c, k)


def test_model_intensity_follows_the_texture(world):
    """The model image of the wall at the true pose is the texture's luminance, to the blur of fusing it into 6 mm voxels."""
    case, true = pc.wall_case()
    c = case.but("at the truth", ref=true)
    I = world.model(c)[2][0]
    live = c.live_tuple()[2][0]
    assert (I >= 0).mean() > 0.99
    err = np.abs(I - live)[I >= 0]
    print(f"wall model intensity vs live: mean |diff| {err.mean():.4f}, worst {err.max():.4f}")
    assert err.mean() < 0.02


# ------------------------------------------------------------------------------------------------------------------------
# J: sign and convention
# ------------------------------------------------------------------------------------------------------------------------
def test_jacobian_predicts_the_residuals_change(world):
    """r(step(M, xi)) - r(M) against J . xi, pair by pair, for a small step along each of the six axes."""
    case, _ = pc.wall_case()
    model, live, P, PP = world.model(case), case.live_tuple(), case.P(), case.PP()
    i0 = {}
    ps.pair_terms(live, model, 0, EYE34[:, :3], EYE34[:, 3], P, PP, i0)
    r0 = dict(zip(i0["idx"].tolist(), zip(i0["r"], i0["J"])))
    for axis in range(6):
        xi = np.zeros(6)
        xi[axis] = 2e-4
        M = ts.step(EYE34, xi)
        i1 = {}
        ps.pair_terms(live, model, 0, M[:, :3].astype(f32), M[:, 3].astype(f32), P, PP, i1)
        got, want = [], []
        for k, r in zip(i1["idx"].tolist(), i1["r"]):
            if k in r0:
                got.append(float(r) - float(r0[k][0]))
                want.append(float(r0[k][1][axis]) * xi[axis])
        got, want = np.array(got), np.array(want)
        assert got.size > 10000
        corr = float(got @ want / np.sqrt((got @ got) * (want @ want)))
        print(f"axis {axis}: {got.size} pairs, correlation of dr with J xi {corr:.4f}, |dr| {np.abs(got).mean():.2e}")
        assert corr > 0.9, (axis, corr)          # a wrong sign gives -1, a wrong axis about 0


def one_step(world, c, level):
    model, live, P, PP = world.model(c), c.live_tuple(), c.P(), c.PP()
    geo, _ = ts.system((c.live, c.mask), model[:2], level, EYE34, P)
    pho, _ = ps.system(live, model, level, EYE34, P, PP)
    xi = ts.cholesky_solve(ps.combine(geo, pho, PP))
    assert xi is not None, c
    before = pho[27] / pho[28]
    s, n = ps.photo_cost(live, model, level, ts.step(EYE34, xi), P, PP)
    return before, s / n, int(pho[28]), n


def test_one_combined_step_lowers_the_photometric_cost(world):
    cases = pc.convergence_cases() + [pc.wall_case()[0]]
    for c in cases:
        for level in range(c.par["n_levels"]):
            before, after, n0, n1 = one_step(world, c, level)
            print(f"{c} level {level}: mean r^2 {before:.3e} -> {after:.3e} ({n0} -> {n1} pairs)")
            assert after < before and n1 > 0.9 * n0, (c, level)


# ------------------------------------------------------------------------------------------------------------------------
# named branches
# ------------------------------------------------------------------------------------------------------------------------
def info_of(world, c):
    info = {}
    terms = pc.spec_terms(world, c, info)
    assert sum(info["rejected"].values()) + len(terms) == info["samples"] == ts.sample_grid(c.hw, c.level)[0].size, c
    assert len(info["idx"]) == len(terms) and np.all(np.diff(info["idx"]) > 0), c
    assert pc.spec_terms(world, c).tobytes() == terms.tobytes(), c              # info changes nothing
    return terms, info


def test_every_branch_case_reaches_its_branch(world):
    for name, (c, gate) in pc.branch_cases().items():
        terms, info = info_of(world, c)
        print(f"{name}: {len(terms)} pairs of {info['samples']}, rejected {info['rejected']}")
        if gate is not None:
            assert info["rejected"][gate] > 0, (name, info["rejected"])
        if name.startswith("footprint off the"):
            assert info["footprint_sides"][name.split()[-1]] > 0, (name, info["footprint_sides"])
        if name == "level too small":
            assert info["samples"] == 1 and len(terms) == 0
        elif name.startswith("plain"):
            assert len(terms) > 0.5 * info["samples"]
        else:
            assert len(terms) > 0, name


def test_occlusion_gate_has_two_sides(world):
    """Moving the camera 3 cm forward makes p2 < t - dist on the wall, 3 cm back p2 > t + dist: both are rejected, and with
    the gate wide open the same poses keep those pairs."""
    cases = pc.branch_cases()
    for name in ("occluded in front", "occluded behind"):
        c = cases[name][0]
        _, tight = info_of(world, c)
        _, wide = info_of(world, c.but("wide", dist=(10.0,) * 3))
        assert wide["rejected"]["occluded"] < tight["rejected"]["occluded"], name
        assert tight["rejected"]["occluded"] > 0.5 * tight["samples"], (name, tight["rejected"])


def test_residual_threshold_at_and_beyond(world):
    at, beyond = pc.threshold_cases(world)
    (ta, ia), (tb, ib) = info_of(world, at), info_of(world, beyond)
    assert len(ta) > len(tb) > 0
    assert np.abs(ia["r"]).max() == f32(at.ithr)                        # |r| == threshold is a pair
    assert np.abs(ib["r"]).max() < f32(at.ithr)
    assert ib["rejected"]["residual"] - ia["rejected"]["residual"] == len(ta) - len(tb)


def test_edge_volume_mixes_valid_and_invalid_intensities(world):
    for c in pc.fill_edge_live(world, pc.edge_cases()):
        I = world.model(c)[2]
        assert 0.02 < (I[0] < 0).mean() < 0.98, c
        terms, info = info_of(world, c)
        assert info["rejected"]["invalid_intensity"] > 0 and len(terms) > 20, (c, info["rejected"], len(terms))


def test_state_cases(world):
    none, zero, few = pc.state_cases()
    h = []
    r = pc.spec_track(world, none, h)
    assert r["photo_pairs"] == 0 and not r["lost"] and all(x["photo_pairs"] == 0 for x in h)
    g = ts.track((none.live, None), world.model(none)[:2], none.P())
    assert np.array_equal(r["M"], g["M"])                                # no photometric pair: the geometric track's steps
    for c in (zero, few):
        r = pc.spec_track(world, c)
        assert r["status"] == 2 and r["pose"].tobytes() == c.ref.tobytes()


def test_tracked_cases_keep_clear_of_the_thresholds(world):
    must = pc.state_cases() + [pc.wall_case()[0]]
    assert len(pc.clear_cases(world, must)) == len(must)
    clear = pc.clear_cases(world, pc.convergence_cases())
    print(f"{len(clear)} of {len(pc.convergence_cases())} convergence candidates are clear: {clear}")
    assert len(clear) >= pc.MIN_CLEAR


# ------------------------------------------------------------------------------------------------------------------------
# the wall
# ------------------------------------------------------------------------------------------------------------------------
def test_the_wall(world):
    case, true = pc.wall_case()
    start = pc.in_plane_error(case.ref, true)
    assert start >= 3.0 * 1.2 / float(pc.K_SMALL[0])
    geo = pc.spec_track(world, case.but("depth only", rgb=None))
    both = pc.spec_track(world, case)
    e_geo, e_both = pc.in_plane_error(geo["pose"], true), pc.in_plane_error(both["pose"], true)
    print(f"wall: guess {start * 1e3:.2f} mm off in the plane; depth only: status {geo['status']}, {e_geo * 1e3:.3f} mm; "
          f"combined (photo_weight {case.weight}): status {both['status']}, {e_both * 1e3:.3f} mm, "
          f"{both['photo_pairs']} photometric pairs, photo rmse {both['photo_rmse']:.4f}")
    assert geo["lost"] or e_geo > 0.5 * start
    assert not both["lost"]
    assert e_both <= pc.VS, e_both


# ------------------------------------------------------------------------------------------------------------------------
# host-only ABI pieces
# ------------------------------------------------------------------------------------------------------------------------
def test_photo_params_default():
    cfg = pc.config()
    p = capi.photo_params_default(cfg)
    assert p.photo_weight == f32(ps.DEFAULT_WEIGHT) and p.intensity_thresh == f32(ps.DEFAULT_ITHR)
    assert capi.load().tsdf_photo_params_default(None, C.byref(p)) == -1
    assert "NULL" in capi.load().tsdf_last_error().decode()


@pytest.mark.parametrize("struct, cname", [(capi.PhotoParams, "tsdf_photo_params"),
                                           (capi.TrackRgbdResult, "tsdf_track_rgbd_result")])
def test_photo_layouts_match_c(tmp_path, struct, cname):
    prog = tmp_path / "layout.c"
    fields = [f for f, _ in struct._fields_]
    body = "\n".join(f'printf("{f} %zu\\n", offsetof({cname}, {f}));' for f in fields)
    prog.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "tsdf_hip.h"\n'
                    f'int main(void){{printf("size %zu\\n", sizeof({cname}));\n' + body + "\nreturn 0;}\n")
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(prog), "-o", str(exe)])
    got = dict(line.split() for line in subprocess.check_output([str(exe)]).decode().splitlines())
    assert int(got["size"]) == C.sizeof(struct)
    for f in fields:
        assert int(got[f]) == getattr(struct, f).offset, f
