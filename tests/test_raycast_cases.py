"""The cases of tests/raycast_cases.py are what they claim, on the CPU (the restatement tests/raycast_spec.py and float64):

  * every class a case names is reached by at least the stated number of its rays, read off the restatement's report ("end",
    the set-up facts, the trace of the march); a class that is not reached fails with the class and the case in the message;
  * every march ends within max_steps, misses follow the convention, no output is NaN;
  * except where a case exists to miss, at least a quarter of its rays hit;
  * for the cases that hold a plane (an unclipped linear field), a float64 ray / plane intersection that shares no code with
    the restatement -- the float32 base2world, cam2world, K and origin widened to float64, the relative pose composed in
    float64 -- gives the hit depth, the camera-frame normal and the label voxel.

tests/test_gpu_raycast_exact.py holds the device to the restatement on the same cases bit for bit, so what is proved here holds
there."""
import numpy as np
import pytest

import raycast_cases as rc
import raycast_spec as rs
from semantic_slam_amd import capi

f32 = np.float32
f64 = np.float64
TINY = np.finfo(f32).tiny

SINGLES = rc.single_cases()
BATCHES = rc.batch_cases()

# Worst errors of the restatement against the float64 geometry over every planar case of SINGLES (all three base frames),
# measured with this file (run it with -s to see them): depth 3.95e-6 voxel, normal 1.32e-7.  The bounds are 4 x that; the
# margin covers the rounding of other pixel sets, not algorithmic slack.  DESIGN.md ("Raycasting") quotes the same figures.
DEPTH_BOUND_VOX = 4 * 3.95e-6
NORMAL_BOUND = 4 * 1.32e-7
LABEL_MARGIN_VOX = 1e-3
LABEL_EXCLUDED_MAX = 0.05


def spec_render(c, report=True):
    return rs.render(c["tsdf"], c["weight"], c["dims"], c["origin"], c["vs"], c["trunc"], c["K"], c["hw"], c["near"], c["far"],
                     c["thr"], rc.cam2base(c, capi), pixels=c["pixels"], label=c["label"], colour=c["colour"], report=report)


_rendered = {}


def rendered(c):
    if c["name"] not in _rendered:
        _rendered[c["name"]] = spec_render(c)
    return _rendered[c["name"]]


def normal_samples(c, o):
    """Validity [n, 6] and values [n, 6] of the six central-difference samples at g* (+x, -x, +y, -y, +z, -z)."""
    g = o["g_hit"].T.astype(f32)
    valid, F = [], []
    for i in range(3):
        for s in (f32(1), f32(-1)):
            p = g.copy()
            p[i] = g[i] + s
            v, x = rs.sample(c["tsdf"], c["weight"], c["dims"], f32(c["thr"]), p)
            valid.append(v)
            F.append(x)
    return np.stack(valid, -1), np.stack(F, -1)


def classify(c, o):
    """{class: bool [n]} of a single-volume case."""
    n = o["hit"].size
    hit, end, ns = o["hit"], o["end"], o["samples"]
    hi = np.array([d - 1 for d in c["dims"]], f32)
    go, gd, gz = o["go"], o["gd"], o["gd_zero"]
    cls = {name: end == k for k, name in enumerate(rs.END)}
    cls["zero_samples"] = ns == 0
    with np.errstate(invalid="ignore", over="ignore"):
        inside_go = (go >= 0) & (go <= hi)
        cls["gd0_all"] = gz.all(1)
        cls["gd0_both_hit"] = (gz.sum(1) == 2) & hit
        cls["gd0_one_hit"] = (gz.sum(1) == 1) & hit
        cls["gd0_on_lo_face_hit"] = (gz & (go == 0)[None]).any(1) & hit
        cls["gd0_on_hi_face_hit"] = (gz & (go == hi)[None]).any(1) & hit
        cls["gd0_outside"] = (gz & ~inside_go[None]).any(1) & cls["setup_miss"]
        cls["touch"] = o["touch"]
        cls["touch_one_sample"] = o["touch"] & (ns == 1) & ~hit
        cls["t_exit_is_far"] = hit & (o["t_exit"] == f32(c["far"]))
        cls["t_enter_is_near_hit"] = hit & (o["t_enter"] == f32(c["near"]))
        cls["go_not_finite"] = np.full(n, not np.isfinite(go).all())
        sub = ((np.abs(gd) > 0) & (np.abs(gd) < TINY)).any(1)
        cls["gd_subnormal_hit"] = sub & hit
        cls["gd_subnormal_setup_miss"] = sub & cls["setup_miss"]

        T = o["trace"]
        t, F, valid = T["t"], T["F"], T["valid"]
        k_max = t.shape[0]
        taken = np.arange(k_max)[:, None] < ns[None]                                  # the samples a ray really took
        g = np.stack([go[i] + t * gd[None, :, i] for i in range(3)], -1).astype(f32)  # [k, n, 3]
        inside = ((g >= 0) & (g <= hi)).all(-1) & taken
        if k_max:
            first_valid, F0 = valid[0], F[0]
        else:
            first_valid, F0 = np.zeros(n, bool), np.zeros(n, f32)
        neg_all = np.where(valid & taken, F <= 0, True).all(0)
        cls["negative_from_the_start"] = first_valid & (F0 <= 0) & neg_all & ~hit
        cls["first_sample_zero"] = first_valid & (F0 == 0) & ~hit
        cls["stall_one_sample"] = cls["stall"] & (ns == 1)
        viv = np.zeros(n, bool)
        for k in range(1, k_max - 1):
            viv |= (valid[k - 1] & (F[k - 1] > 0) & ~valid[k] & taken[k] & valid[k + 1] & (F[k + 1] <= 0))
        cls["valid_invalid_valid"] = viv & ~hit
        cls["overflow_invalid"] = (inside & ~valid & ~np.isfinite(F)).any(0)
        cls["weight_invalid"] = (inside & ~valid & np.isfinite(F)).any(0)
        rays = np.arange(n)
        kh = np.clip(ns - 1, 0, max(k_max - 1, 0))
        if k_max:
            Fh, Fp, th = F[kh, rays], F[np.clip(kh - 1, 0, None), rays], t[kh, rays]
        else:
            Fh = Fp = th = np.zeros(n, f32)
        ratio_one = hit & (Fh == 0) & (o["depth"] == th)
        cls["hit_at_positive_zero"] = ratio_one & ~np.signbit(Fh)
        cls["hit_at_negative_zero"] = ratio_one & np.signbit(Fh)
        cls["hit_subnormal"] = hit & (np.abs(Fh) < TINY) & (Fh != 0) & (Fp > 0) & (Fp < TINY)
        gs = o["g_hit"]
        cls["hit_in_cell_2"] = hit & (gs[:, 2] >= 2) & (gs[:, 2] <= 3)

        nv, nF = normal_samples(c, o)
        nrm = o["normal"]
        nz = hit & (nrm == 0).all(1)
        cls["normal_unit"] = hit & (np.abs(np.linalg.norm(nrm.astype(f64), axis=1) - 1) < 1e-5)
        R, _ = rs.pose_parts(rc.cam2base(c, capi), c["origin"], c["vs"])
        nn = [nF[:, 2 * i] - nF[:, 2 * i + 1] for i in range(3)]
        m = [(R[0, j] * nn[0] + R[1, j] * nn[1]) + R[2, j] * nn[2] for j in range(3)]
        ln = np.sqrt((m[0] * m[0] + m[1] * m[1]) + m[2] * m[2])
        cls["len_zero"] = nz & nv.all(1) & (ln == 0)
        cls["len_not_finite"] = nz & nv.all(1) & ~np.isfinite(ln)
        deep = ((gs >= 1) & (gs <= hi - 1)).all(1)
        cls["normal_zero_interior"] = nz & deep & ~nv.all(1)
        for i, ax in enumerate("xyz"):
            cls[f"normal_zero_near_lo_{ax}"] = nz & (gs[:, i] < 1)
            cls[f"normal_zero_near_hi_{ax}"] = nz & (gs[:, i] > hi[i] - 1)
            cls[f"vox_lo_{ax}"] = hit & (gs[:, i] < f32(0.5))
            cls[f"vox_hi_{ax}"] = hit & (gs[:, i] > hi[i] - f32(0.5))
            x = (gs[:, i] + f32(0.5)).astype(f32)
            cls[f"floor_tie_{ax}"] = hit & (x == np.floor(x))
    return cls


def assert_conventions(c, o, dims):
    assert o["samples"].max() <= rs.max_steps(dims), c["name"]
    miss = ~o["hit"]
    for k in ("depth", "normal", "label", "colour"):
        if k in o:
            assert not np.isnan(o[k].astype(f64)).any(), f"{c['name']}: NaN in {k}"
            assert not o[k][miss].any(), f"{c['name']}: a miss with a non-zero {k}"
    assert not np.signbit(o["depth"][miss]).any(), f"{c['name']}: a miss with depth -0"
    assert np.all(o["depth"][o["hit"]] >= f32(c["near"])) and np.all(o["depth"][o["hit"]] <= f32(c["far"])), c["name"]


def test_sizes_and_shapes():
    """The limits of the issue, and every grid and image shape it names is used."""
    for c in SINGLES:
        assert c["dims"][0] <= 33 and c["dims"][1] <= 20 and c["dims"][2] <= 17, c["name"]
        assert c["hw"][0] <= 33 and c["hw"][1] <= 40, c["name"]
    for b in BATCHES:
        assert 1 <= len(b["members"]) <= 5 and b["hw"][0] <= 33 and b["hw"][1] <= 40
    assert {c["dims"] for c in SINGLES} >= set(rc.GRIDS)
    assert {c["hw"] for c in SINGLES} >= set(rc.IMAGES)
    assert any(not np.array_equal(c["base2world"], np.eye(4, dtype=f32)) for c in SINGLES)
    assert all((c["label"] is not None) <= (c["dims"] in rc.LABEL_GRIDS) for c in SINGLES)
    assert sum(c["label"] is not None for c in SINGLES) >= 30


@pytest.mark.parametrize("c", SINGLES, ids=[c["name"] for c in SINGLES])
def test_case_reaches_its_classes(c):
    o = rendered(c)
    assert_conventions(c, o, c["dims"])
    cls = classify(c, o)
    for name, least in c["expect"].items():
        got = int(cls[name].sum())
        assert got >= least, f"class '{name}' is reached by {got} rays of case '{c['name']}' ({c['branch']}); it needs {least}"
    for name in c["never"]:
        assert not cls[name].any(), f"class '{name}' is reached by {int(cls[name].sum())} rays of case '{c['name']}', which excludes it"
    if not c["miss"]:
        share = o["hit"].mean()
        assert share >= 0.25, f"case '{c['name']}': only {share:.0%} of its rays hit"


# ------------------------------------------------------------------------------------------------------------------------
# the float64 geometry
# ------------------------------------------------------------------------------------------------------------------------
def plane_geometry(c):
    """Depth (voxels), camera-frame normal, nearest voxel and its distance from a rounding boundary of every ray against the
    case's plane: all in float64, from the float32 inputs widened."""
    h, w = c["hw"]
    vv, uu = np.mgrid[0:h, 0:w]
    u, v = uu.ravel().astype(f64), vv.ravel().astype(f64)
    K = c["K"].astype(f64)
    c2b = np.linalg.inv(c["base2world"].astype(f64)) @ c["cam2world"].astype(f64).reshape(4, 4)
    vs = f64(f32(c["vs"]))
    d_cam = np.stack([(u - K[2]) / K[0], (v - K[5]) / K[4], np.ones_like(u)])
    gd = (c2b[:3, :3] @ d_cam) / vs
    go = ((c2b[:3, 3] - c["origin"].astype(f64)) / vs)[:, None]
    n, d = c["plane"]
    n = np.asarray(n, f64)
    with np.errstate(divide="ignore", invalid="ignore"):
        t = (d - n @ go) / (n @ gd)                                   # camera z of the intersection, metres
        p = go + t * gd
    normal = -(c2b[:3, :3].T @ n)
    normal /= np.linalg.norm(normal)
    near_vox = np.floor(p + 0.5)
    frac = (p + 0.5) - near_vox
    margin = np.minimum(frac, 1 - frac).min(0)
    dims = c["dims"]
    near_vox = np.clip(near_vox, 0, np.array([x - 1 for x in dims], f64)[:, None])
    vox = (near_vox[2] * dims[1] + near_vox[1]) * dims[0] + near_vox[0]
    return t / vs, normal, vox, margin


PLANAR = [c for c in SINGLES if c["plane"] is not None]


def test_planes_against_float64_geometry():
    worst_d = worst_n = 0.0
    assert len(PLANAR) >= 30 and sum(not np.array_equal(c["base2world"], np.eye(4, dtype=f32)) for c in PLANAR) >= 20
    for c in PLANAR:
        o = rendered(c)
        hit = o["hit"]
        depth, normal, vox, margin = plane_geometry(c)
        assert hit.sum() > 0, c["name"]
        err = np.abs(o["depth"][hit].astype(f64) / f64(f32(c["vs"])) - depth[hit])
        assert err.max() <= DEPTH_BOUND_VOX, f"{c['name']}: depth off by {err.max():.3g} voxel at ray {np.nonzero(hit)[0][err.argmax()]}"
        worst_d = max(worst_d, err.max())
        unit = hit & (o["normal"] != 0).any(1)
        if unit.any():
            en = np.abs(o["normal"][unit].astype(f64) - normal[None]).max()
            assert en <= NORMAL_BOUND, f"{c['name']}: normal off by {en:.3g}"
            worst_n = max(worst_n, en)
        if c["label"] is not None and c["f64_labels"]:
            sure = hit & (margin > LABEL_MARGIN_VOX)
            excluded = 1 - sure.sum() / hit.sum()
            assert excluded <= LABEL_EXCLUDED_MAX, f"{c['name']}: {excluded:.1%} of the hits lie within {LABEL_MARGIN_VOX} voxel of a rounding boundary (cap {LABEL_EXCLUDED_MAX:.0%})"
            want = vox[sure].astype(np.int64)
            assert np.array_equal(o["label"][sure], (want % 65535).astype(np.uint16)), c["name"]
            assert np.array_equal(o["colour"][sure], want.astype(np.uint32)), c["name"]
    print(f"float64 geometry over {len(PLANAR)} planar cases: worst depth error {worst_d:.3g} voxel, worst normal error {worst_n:.3g}")


# ------------------------------------------------------------------------------------------------------------------------
# batch
# ------------------------------------------------------------------------------------------------------------------------
def batch_members(b):
    return [dict(m, cam2base=capi.multiply_matrix(capi.invert_matrix(m["base2world"])[1], b["cam2world"])) for m in b["members"]]


def spec_batch(b, report=True):
    return rs.render_batch(batch_members(b), b["K"], b["hw"], b["near"], b["far"], b["thr"], report=report)


def classify_batch(b, o):
    """The kernel's member loop over the members' own renders: who wins, and which comparisons were at equality."""
    outs = o["members"]
    n = o["depth"].size
    best, who = np.zeros(n, f32), np.full(n, -1)
    cls = {k: np.zeros(n, bool) for k in ("tie", "replaced", "culled", "t_enter_equals_best", "t_enter_ulp_below_best")}
    for i, m in enumerate(outs):
        ok = m["end"] != rs.END.index("setup_miss")
        have = who >= 0
        cull = ok & have & ~(m["t_enter"] < best)
        cls["culled"] |= cull
        cls["t_enter_equals_best"] |= ok & have & (m["t_enter"] == best)
        cls["t_enter_ulp_below_best"] |= ok & have & (np.nextafter(m["t_enter"], f32(np.inf)) == best)
        marched = ok & ~cull & m["hit"]
        cls["tie"] |= marched & have & (m["depth"] == best)
        win = marched & (~have | (m["depth"] < best))
        cls["replaced"] |= win & have
        best = np.where(win, m["depth"], best)
        who = np.where(win, i, who)
    assert np.array_equal(who, o["member"]), b["name"]
    for i in range(len(outs)):
        cls[f"member_{i}"] = who == i
    seen = len(set(who[who >= 0].tolist()))
    for k in range(1, 6):
        cls[f"members_seen_{k}"] = np.full(n, seen >= k)
    return cls


@pytest.mark.parametrize("b", BATCHES, ids=[b["name"] for b in BATCHES])
def test_batch_case_reaches_its_classes(b):
    o = spec_batch(b)
    for m, mo in zip(b["members"], o["members"]):
        assert mo["samples"].max() <= rs.max_steps(m["dims"]), b["name"]
    assert not np.isnan(o["depth"]).any() and not np.isnan(o["normal"]).any()
    miss = o["member"] < 0
    assert not o["depth"][miss].any() and not o["normal"][miss].any()
    cls = classify_batch(b, o)
    for name, least in b["expect"].items():
        got = int(cls[name].sum())
        assert got >= least, f"class '{name}' is reached by {got} rays of batch case '{b['name']}' ({b['branch']}); it needs {least}"
    if not b["miss"]:
        assert (~miss).mean() >= 0.25, f"batch case '{b['name']}': only {(~miss).mean():.0%} of its rays hit"


def test_twins_tie_whichever_comes_first():
    """Swapping two members that are identical in configuration and contents changes nothing: index 0 wins every hit."""
    b = next(x for x in BATCHES if x["name"] == "twins")
    o = spec_batch(b)
    swapped = dict(b, members=b["members"][::-1])
    s = spec_batch(swapped)
    assert (o["member"] >= 0).sum() >= 64 and not (o["member"] > 0).any() and not (s["member"] > 0).any()
    assert o["depth"].tobytes() == s["depth"].tobytes()
