"""The named cases that hold raycasting (csrc/tsdf_raycast.hip.h) to its rule at ray, box, march, value and batch edges
(test infrastructure; no device and no torch).  tests/test_raycast_cases.py proves on the CPU, with the restatement
(tests/raycast_spec.py) and an independent float64 ray / plane intersection, that each case reaches the branch it is named for;
tests/test_gpu_raycast_exact.py renders every case on the device and compares all 32 bits.

A case is a dict:
    name, branch      what it is called and the branch of the rule it exists for
    dims, vs, origin, trunc, base2world          the grid (a volume is created once per distinct grid, grid_key())
    tsdf, weight, label, colour                  the uploaded state (label / colour: None where the case renders neither)
    K, hw, near, far, thr, cam2world, pixels     the camera (pixels: None = every pixel)
    expect            {class: least number of rays that must reach it}; the classes are those of classify()
    never             classes no ray may reach
    miss              True when the case exists to miss (exempt from "a quarter of the rays hit")
    plane             (n, d) of the unclipped linear field tsdf = (d - n . g) / scale (grid units, |n| = 1), or None
    f64_labels        whether the float64 label check applies (not where the plane sits on a rounding boundary by design)
    tilt              whether the case is repeated under the tilted base frame (not where only exact coincidences make it)

Every grid is at most 33 x 20 x 12 voxels and every image at most 40 x 33 pixels.  Voxel size, origins and most poses are
dyadic, so go = (T - origin) / vs is exact and a camera "on a face" is on it bit for bit.

Label / colour voxel: a hit lies inside [0, hi] on every axis, so floorf(g* + 0.5) is already in [0, hi] and the clamp of the rule
never changes a value here; the cases with hits within half a voxel of a face ("vox_lo_*", "vox_hi_*") hold the rounding beside
the clamp, not the clamp."""
import numpy as np

f32 = np.float32
f64 = np.float64

VS = f32(0.0625)
ORIGIN = np.array([-0.5, -0.25, 1.0], f32)
DEFAULT_TRUNC = float(VS * f32(5))
I3 = np.eye(3)
# camera z along base +x / +y (camera x, y follow cyclically): db = (1, dcx, dcy) and (dcy, 1, dcx)
LOOK = {"z": I3, "x": np.array([[0.0, 0, 1], [1, 0, 0], [0, 1, 0]]), "y": np.array([[0.0, 1, 0], [0, 0, 1], [1, 0, 0]])}
AXES = {"z": (2, 0, 1), "x": (0, 1, 2), "y": (1, 2, 0)}           # (axis of camera z, of camera x, of camera y)

GRIDS = [(2, 2, 2), (2, 3, 17), (17, 2, 3), (3, 17, 2), (9, 7, 5), (33, 20, 12)]
# tsdf_labels_enable and tsdf_colour_enable take grids whose dim_x is a multiple of 4 only (tests/test_gpu_raycast_exact.py
# asserts the refusal on a grid of GRIDS), so label and colour ride on these neighbours of GRIDS: the shape cases, the normal
# and the label-voxel cases.  A case on any other grid renders depth and normal alone.
LABEL_GRIDS = [(4, 3, 17), (8, 7, 5), (32, 20, 12)]
IMAGES = [(1, 1), (1, 40), (33, 1), (15, 17), (16, 16), (17, 33)]     # (h, w)

# a quarter turn about z plus a dyadic translation: inverting it and composing with a dyadic pose is exact in float32, so the
# classes of a case survive the change of frame bit for bit
BASE_QUARTER = np.array([[0, -1, 0, 0.75], [1, 0, 0, -1.5], [0, 0, 1, 0.25], [0, 0, 0, 1]], f64)


def rot(axis, angle):
    a = np.asarray(axis, f64) / np.linalg.norm(axis)
    Kx = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * Kx + (1 - np.cos(angle)) * (Kx @ Kx)


BASE_TILT = np.eye(4)
BASE_TILT[:3, :3] = rot([0.3, -1.0, 0.5], 0.7)
BASE_TILT[:3, 3] = [0.31, -0.77, 0.42]


def pose(R, T):
    m = np.eye(4)
    m[:3, :3] = R
    m[:3, 3] = T
    return m


def cam_at(go, R=I3, origin=ORIGIN, vs=VS):
    """cam2base of a camera at grid point go with rotation R (float64; exact where go, origin and vs are dyadic)."""
    return pose(R, np.asarray(origin, f64) + f64(vs) * np.asarray(go, f64))


def intrinsics(fx, fy, cx, cy):
    return np.array([fx, 0, cx, 0, fy, cy, 0, 0, 1], f32)


def voxel_index(dims):
    return np.arange(int(np.prod(dims)), dtype=np.int64)


def voxel_coords(dims):
    """i, j, k of every voxel, flat and x-fastest."""
    k, j, i = np.meshgrid(np.arange(dims[2]), np.arange(dims[1]), np.arange(dims[0]), indexing="ij")
    return i.ravel(), j.ravel(), k.ravel()


def plane_state(dims, n, d, scale=5.0, weight=2.0):
    """tsdf = (d - n . (i, j, k)) / scale, unclipped; weights all `weight`."""
    i, j, k = voxel_coords(dims)
    n = np.asarray(n, f64)
    t = (d - (n[0] * i + n[1] * j + n[2] * k)) / scale
    return t.astype(f32), np.full(t.size, weight, f32)


def layer_state(dims, axis, profile, weight=2.0):
    """tsdf constant over each layer of `axis`: profile[index along the axis]."""
    idx = voxel_coords(dims)[axis]
    t = np.asarray(profile, f32)[idx]
    return t, np.full(t.size, weight, f32)


def ids(dims):
    """A distinct label and colour per voxel: the index (modulo 65535 for the uint16 label)."""
    v = voxel_index(dims)
    return (v % 65535).astype(np.uint16), v.astype(np.uint32)


def case(name, branch, dims, state, K, hw, c2b, *, vs=VS, origin=ORIGIN, trunc=DEFAULT_TRUNC, near=0.0, far=6.0, thr=0.9,
         base=None, ids_too=False, pixels=None, expect=None, never=(), miss=False, plane=None, f64_labels=True, tilt=True):
    tsdf, weight = state
    b2w = np.eye(4) if base is None else np.asarray(base, f64)
    with np.errstate(invalid="ignore", over="ignore"):
        c2w = (b2w @ np.asarray(c2b, f64)).astype(f32)
    label, colour = ids(dims) if ids_too and dims[0] % 4 == 0 else (None, None)      # see LABEL_GRIDS
    return dict(name=name, branch=branch, dims=tuple(int(d) for d in dims), vs=float(vs), origin=np.asarray(origin, f32),
                trunc=float(trunc), base2world=b2w.astype(f32), tsdf=np.asarray(tsdf, f32), weight=np.asarray(weight, f32),
                label=label, colour=colour, K=np.asarray(K, f32), hw=tuple(hw), near=float(near), far=float(far),
                thr=float(thr), cam2world=c2w, pixels=pixels, expect=dict(expect or {}), never=tuple(never), miss=miss,
                plane=plane, f64_labels=f64_labels, tilt=tilt)


def rebased(c, base, tag, keep_classes=True):
    """The same case seen from a volume whose base frame is `base`: cam2world = base * (the case's cam2base)."""
    assert np.array_equal(c["base2world"], np.eye(4, dtype=f32))
    out = dict(c)
    out["name"] = f"{c['name']} [{tag}]"
    out["base2world"] = np.asarray(base, f64).astype(f32)
    with np.errstate(invalid="ignore", over="ignore"):
        out["cam2world"] = (np.asarray(base, f64) @ c["cam2world"].astype(f64)).astype(f32)
    if not keep_classes:                     # an inexact frame keeps the geometry, not the bit-level coincidences
        out["expect"] = {k: v for k, v in c["expect"].items() if k in ("hit", "setup_miss")}
        out["never"] = ()
    return out


def grid_key(c):
    return (c["dims"], c["vs"], tuple(float(x) for x in c["origin"]), c["trunc"], c["base2world"].tobytes())


def cam2base(c, capi):
    """inverse(base2world) * cam2world through the library's own host functions, as tsdf_create and compose_cam2base do."""
    return capi.multiply_matrix(capi.invert_matrix(c["base2world"])[1], c["cam2world"])


# ------------------------------------------------------------------------------------------------------------------------
# views
# ------------------------------------------------------------------------------------------------------------------------
def front_view(dims, hw, look="z", dist=6.0, surf=None, fill=1.3, integer_centre=False):
    """A camera `dist` voxels outside the low face of the look axis, centred on the other two, whose image spans `fill`
    times the grid at the depth of a surface `surf` voxels inside.  Returns (K, cam2base go, R)."""
    a, b, c = AXES[look]
    h, w = hw
    surf = (dims[a] - 1) / 2 if surf is None else surf
    s = dist + surf
    fill_x, fill_y = fill if isinstance(fill, tuple) else (fill, fill)
    fx = max(w, 2) * s / (fill_x * (dims[b] - 1))
    fy = max(h, 2) * s / (fill_y * (dims[c] - 1))
    cx, cy = (w - 1) / 2, (h - 1) / 2
    if integer_centre:
        cx, cy = float(w // 2), float(h // 2)
    go = np.zeros(3)
    go[a], go[b], go[c] = -dist, (dims[b] - 1) / 2, (dims[c] - 1) / 2
    return intrinsics(fx, fy, cx, cy), go, LOOK[look]


def tilted_plane(dims, look, tilt=(0.12, -0.17), depth=None):
    """(n, d): a plane facing a camera that looks along `look`, tilted by tilt (radians, about the two image axes),
    through the grid's centre line at `depth` voxels along the look axis."""
    a, b, c = AXES[look]
    n = np.zeros(3)
    n[a], n[b], n[c] = 1.0, np.tan(tilt[0]), np.tan(tilt[1])
    n /= np.linalg.norm(n)
    p = np.array([(d - 1) / 2 for d in dims], f64)
    p[a] = (dims[a] - 1) * 0.55 if depth is None else depth
    return n, float(n @ p)


# ------------------------------------------------------------------------------------------------------------------------
# families
# ------------------------------------------------------------------------------------------------------------------------
# the centre line of an axis with an even number of voxels is a rounding boundary of the label voxel: the shape cases look from
# a fifth of a voxel beside it
OFF_CENTRE = {"z": np.array([-0.2, 0.2, 0.0]), "x": np.array([0.0, -0.2, 0.2]), "y": np.array([0.2, 0.0, -0.2])}


def shape_cases():
    """Every grid shape under an image shape, a tilted plane with labels and colour: partial 8 x 8 tiles and 16 x 16
    workgroups in each direction, dim_i - 2 == 0 on each axis, and the float64 geometry."""
    out = []
    looks = ["z", "z", "z", "z", "x", "y"]
    for dims, hw, look in zip(GRIDS, IMAGES, looks):
        thin = min(dims) <= 3
        n, d = tilted_plane(dims, look, tilt=(0.05, -0.04) if thin else (0.2, -0.17))
        a = AXES[look][0]
        K, go, R = front_view(dims, hw, look, surf=(dims[a] - 1) * 0.55)
        go = go + OFF_CENTRE[look]
        out.append(case(f"shape {dims} {hw[1]}x{hw[0]} look {look}", "grid and image shapes", dims, plane_state(dims, n, d), K, hw,
                        cam_at(go, R), ids_too=True, expect={"hit": 1}, plane=(n, d)))
    # the other image shapes on the two grids with room for them, and the other looks
    for dims, hw, look in [((9, 7, 5), (15, 17), "y"), ((9, 7, 5), (17, 33), "z"), ((33, 20, 12), (15, 17), "z"),
                           ((33, 20, 12), (33, 40), "x"), ((33, 20, 12), (16, 16), "y"), ((4, 3, 17), (16, 16), "z"),
                           ((8, 7, 5), (15, 17), "x"), ((8, 7, 5), (17, 33), "z"), ((32, 20, 12), (17, 33), "y"),
                           ((32, 20, 12), (15, 17), "z")]:
        n, d = tilted_plane(dims, look, tilt=(0.2, -0.17))
        a = AXES[look][0]
        K, go, R = front_view(dims, hw, look, surf=(dims[a] - 1) * 0.55)
        out.append(case(f"shape {dims} {hw[1]}x{hw[0]} look {look}", "grid and image shapes", dims, plane_state(dims, n, d), K, hw,
                        cam_at(go + OFF_CENTRE[look], R), ids_too=True, expect={"hit": 1}, plane=(n, d)))
    return out


SETUP_DIMS = (9, 7, 5)


def setup_state(look):
    """A plane square to the look axis a little past the middle of SETUP_DIMS."""
    a = AXES[look][0]
    n = np.zeros(3)
    n[a] = 1.0
    return plane_state(SETUP_DIMS, n, (SETUP_DIMS[a] - 1) * 0.55), (n, (SETUP_DIMS[a] - 1) * 0.55)


def axis_parallel_cases():
    """Identity and quarter-turn rotations with integer cx, cy: the centre column has gd == 0 on the camera-x axis, the
    centre row on the camera-y axis, the centre pixel on both.  The camera sits inside on those axes, on the faces
    go_i == 0 and go_i == hi_i exactly, and one voxel outside."""
    out = []
    hw = (17, 15)
    for look in ("z", "x", "y"):
        a, b, c = AXES[look]
        state, plane = setup_state(look)
        hi = [d - 1 for d in SETUP_DIMS]
        K, go0, R = front_view(SETUP_DIMS, hw, look, surf=plane[1], integer_centre=True)
        for place, gb, gc, exp, nev in (
                ("inside", hi[b] / 2, hi[c] / 2, {"gd0_both_hit": 1, "gd0_one_hit": 8}, ("gd0_outside",)),
                ("on the low faces", 0.0, 0.0, {"gd0_on_lo_face_hit": 8, "gd0_both_hit": 1}, ("gd0_outside",)),
                ("on the high faces", hi[b], hi[c], {"gd0_on_hi_face_hit": 8, "gd0_both_hit": 1}, ("gd0_outside",)),
                ("one voxel outside", -1.0, hi[c] + 1.0, {"gd0_outside": 8}, ("gd0_both_hit",))):
            go = go0.copy()
            go[b], go[c] = gb, gc
            out.append(case(f"axis-parallel look {look}, camera {place}", "gd_i == 0", SETUP_DIMS, state, K, hw, cam_at(go, R),
                            ids_too=True, expect=exp, never=nev, plane=plane, miss=place == "one voxel outside", tilt=place == "inside"))
    return out


def box_cases():
    out = []
    state, plane = setup_state("z")
    # a ray through the edge x = hi, z = 0 (the column u = 15) and through the corner (hi_x, hi_y, 0) (the pixel (15, 15)):
    # go + 6 * (0.5, 0.5, 1) = (8, 6, 0), every quantity dyadic, so t_enter == t_exit == 0.375 exactly
    K = intrinsics(16, 16, 7, 7)
    out.append(case("ray through a box edge and a corner", "t_enter == t_exit", SETUP_DIMS, state, K, (16, 16),
                    cam_at([5, 3, -6]), ids_too=True, expect={"touch": 16, "touch_one_sample": 16}, plane=plane))
    K, go, R = front_view(SETUP_DIMS, (17, 15), "z", surf=plane[1], integer_centre=True)
    out.append(case("camera facing away", "no box ahead", SETUP_DIMS, state, K, (17, 15), cam_at(go, np.diag([-1.0, 1, -1])),
                    expect={"setup_miss": 255}, never=("hit",), miss=True))
    # far face at camera z = (4 + 6) * vs = 0.625
    out.append(case("near beyond the far face", "t_enter > t_exit from near", SETUP_DIMS, state, K, (17, 15), cam_at(go),
                    near=0.64, expect={"setup_miss": 255}, never=("hit",), miss=True))
    # the surface is at camera z = (2.2 + 6) * vs = 0.5125
    out.append(case("far before the surface", "t_exit from far", SETUP_DIMS, state, K, (17, 15), cam_at(go), far=0.5,
                    expect={"exit": 100}, never=("hit",), miss=True))
    out.append(case("far one step past the surface", "t_exit from far", SETUP_DIMS, state, K, (17, 15), cam_at(go),
                    far=0.5125 + 0.0625, ids_too=True, expect={"hit": 64, "t_exit_is_far": 64}, plane=plane))
    # box entry at 0.375; near = 0.375 + 1.37 voxels falls between the second and third sample of the default march
    out.append(case("near between two samples", "t_enter == near", SETUP_DIMS, state, K, (17, 15), cam_at(go),
                    near=0.375 + 1.37 * 0.0625, ids_too=True, expect={"t_enter_is_near_hit": 64}, plane=plane))
    out.append(case("fx negative", "mirrored image", SETUP_DIMS, state, K * np.array([-1, 1, 1, 1, 1, 1, 1, 1, 1], f32), (17, 15),
                    cam_at(go), ids_too=True, expect={"hit": 64}, plane=plane))
    # cx, cy far outside the image: every ray leans by about (0.5, -0.4); the camera is moved so that they still meet the box
    s = 6 + plane[1]
    lean = np.array([(7 + 20.0) / 40.0, (8 - 24.0) / 40.0, 0.0])     # direction of the centre pixel per unit camera z
    out.append(case("cx, cy far outside the image", "oblique rays", SETUP_DIMS, state, intrinsics(40.0, 40.0, -20.0, 24.0), (17, 15),
                    cam_at(go - s * lean), ids_too=True, expect={"hit": 64}, plane=plane))
    return out


INSIDE_DIMS = (33, 20, 12)


def inside_and_singular_cases():
    out = []
    n, d = np.array([0.0, 0, 1]), 6.3
    state = plane_state(INSIDE_DIMS, n, d)
    hw = (15, 17)
    K = intrinsics(12.0, 12.0, 8.0, 7.0)
    mid = [16.0, 9.25]               # off the centre line g_y = 9.5, a rounding boundary of the label voxel
    out.append(case("camera inside, in front of the surface", "t_enter == near inside the box", INSIDE_DIMS, state, K, hw,
                    cam_at([*mid, 1.0]), ids_too=True, expect={"hit": 64, "t_enter_is_near_hit": 64}, plane=(n, d)))
    out.append(case("camera inside, behind the surface", "F <= 0 from the first sample: step vs, no hit", INSIDE_DIMS, state, K,
                    hw, cam_at([*mid, 8.0]), expect={"negative_from_the_start": 200}, never=("hit",), miss=True))
    Z = np.zeros((3, 3))
    out.append(case("R = 0, T outside the box", "gd == 0 on every axis, go outside", INSIDE_DIMS, state, K, hw,
                    cam_at([*mid, -3.0], Z), expect={"setup_miss": 255, "gd0_all": 255}, never=("hit",), miss=True))
    out.append(case("R = 0, T inside in front of the surface", "gd == 0 on every axis: the march stands still in space",
                    INSIDE_DIMS, state, K, hw, cam_at([*mid, 2.0], Z), expect={"gd0_all": 255, "exit": 255}, never=("hit",),
                    miss=True))
    out.append(case("R = 0, T inside behind the surface", "gd == 0 on every axis, F <= 0", INSIDE_DIMS, state, K, hw,
                    cam_at([*mid, 9.0], Z), expect={"gd0_all": 255, "negative_from_the_start": 255}, never=("hit",), miss=True))
    return out


def nonfinite_pose_cases():
    out = []
    state, plane = setup_state("z")
    K, go, R = front_view(SETUP_DIMS, (17, 15), "z", surf=plane[1], integer_centre=True)
    good = cam_at(go)
    far_away = good.copy()
    far_away[0, 3] = 3e38
    out.append(case("translation of 3e38", "go overflows to inf", SETUP_DIMS, state, K, (17, 15), far_away,
                    expect={"setup_miss": 255, "zero_samples": 255, "go_not_finite": 255}, never=("hit",), miss=True))
    for what, (r, c), v in (("NaN in the rotation", (1, 0), np.nan), ("inf in the rotation", (2, 2), np.inf),
                            ("NaN in the translation", (2, 3), np.nan), ("-inf in the translation", (1, 3), -np.inf)):
        m = good.copy()
        m[r, c] = v
        exp = {"setup_miss": 255} if "translation" in what or "inf in" in what else {"setup_miss": 200}
        out.append(case(what, "a go_i or gd_i that is not finite", SETUP_DIMS, state, K, (17, 15), m, expect=exp, never=("hit",),
                        miss=True))
    # db_x = 1e-40 * dcx is subnormal and so is gd_x = db_x / vs; the camera is on the face go_x == 0, so left of the centre
    # column g_x < 0 by a subnormal (no ray may enter), right of it g_x is a positive subnormal (inside).  A build that
    # flushes subnormals sees gd_x == 0 and go_x inside on every column.
    Rs = np.diag([1e-40, 1.0, 1.0])
    g = go.copy()
    g[0] = 0.0
    out.append(case("rotation scaled so that db_x is subnormal", "subnormal gd_i", SETUP_DIMS, state, K, (17, 15), cam_at(g, Rs),
                    ids_too=True, expect={"gd_subnormal_hit": 64, "gd_subnormal_setup_miss": 64}, plane=plane, tilt=False))
    return out


def march_cases():
    out = []
    dims = SETUP_DIMS
    n_vox = int(np.prod(dims))
    K, go, R = front_view(dims, (17, 15), "z", integer_centre=True)
    empty = (np.ones(n_vox, f32), np.zeros(n_vox, f32))
    out.append(case("empty volume, trunc = 0.05 vs", "max_steps", dims, empty, K, (17, 15), cam_at(go), trunc=float(f32(0.05) * VS),
                    expect={"cap": 100}, never=("hit",), miss=True))
    # 1e6 m away: t_enter == 1e6, where ulp(t) = 0.0625 m; vs = 1 / 256 m and s_free = 0.8 * 5 / 256 m are below half of it
    vs = f32(1 / 256)
    origin = np.array([-4 / 256, -3 / 256, 0.0], f32)
    state = plane_state(dims, [0, 0, 1], 2.2)
    out.append(case("camera 1e6 m away", "!(t' > t) after one sample", dims, state, intrinsics(1e9, 1e9, 7, 8), (17, 15),
                    pose(I3, [0.0, 0.0, -1e6]), vs=vs, origin=origin, trunc=float(vs * f32(5)), far=3e6,
                    expect={"stall_one_sample": 200}, never=("hit",), miss=True))
    # F > 0 up to k = 5, a layer of zero weight at k = 6 (the cells j_z = 5 and 6 are invalid), F <= 0 behind it
    d = INSIDE_DIMS
    t, w = plane_state(d, [0, 0, 1], 6.5)
    w[voxel_coords(d)[2] == 6] = 0.0
    Kd, god, _ = front_view(d, (15, 17), "z", surf=6.5)
    out.append(case("a slab of zero weight across the crossing", "valid, invalid, valid: prev_valid is false", d, (t, w), Kd,
                    (15, 17), cam_at(god), expect={"valid_invalid_valid": 100}, never=("hit",), miss=True))
    # tsdf exactly +0 on the layers k = 6 and 7: every sample with g_z in [6, 7] has F == +0 (a -0 cannot come out of the
    # interpolation of equal corners: -0 + f * (+0) = +0)
    prof = [(6 - k) / 5 if k < 6 else (0.0 if k < 8 else (7 - k) / 5) for k in range(d[2])]
    zero_slab = layer_state(d, 2, prof)
    out.append(case("F == +0 at a sample", "F_prev > 0, F == +0: a hit with ratio 1", d, zero_slab, Kd, (15, 17), cam_at(god),
                    ids_too=True, expect={"hit_at_positive_zero": 64}))
    # the first sample (t_enter == near) already lies in the zero slab: camera z of g_z = 6.5 is (6 + 6.5) * vs
    out.append(case("F == 0 at the first sample", "F == 0 without a valid F_prev > 0: no hit", d, zero_slab, Kd, (15, 17), cam_at(god),
                    near=12.5 * 0.0625, expect={"first_sample_zero": 100}, never=("hit",), miss=True))
    # F == -0: the field falls along x, y and z and the sample sits on the voxel (4, 3, 2) itself, whose value is -0; then
    # every f_i == 0 and f_i * (negative) == -0, so F == -0 + -0.  Only the centre ray (gd_x == gd_y == 0, steps of exactly vs)
    # lands on a voxel, so this class has one ray.
    i, j, k = voxel_coords(dims)
    t = ((9 - (i + j + k)) / 128).astype(f32)
    t[(i == 4) & (j == 3) & (k == 2)] = -0.0
    Kc, goc, _ = front_view(dims, (17, 15), "z", surf=2.0, integer_centre=True)
    goc[0], goc[1] = 4.0, 3.0
    out.append(case("F == -0 at a sample", "F_prev > 0, F == -0: a hit with ratio 1", dims, (t, np.full(t.size, 2.0, f32)), Kc,
                    (17, 15), cam_at(goc), ids_too=True, expect={"hit_at_negative_zero": 1, "hit": 64}))
    return out


def value_cases():
    out = []
    dims = SETUP_DIMS
    K, go, R = front_view(dims, (11, 15), "z", surf=2.5, fill=1.1)
    sub = layer_state(dims, 2, [1e-40, 1e-40, 3e-41, -2e-41, -2e-41])
    out.append(case("subnormal tsdf on both sides of the crossing", "subnormal F_prev and F; len == 0 by underflow", dims, sub, K,
                    (11, 15), cam_at(go), ids_too=True, expect={"hit_subnormal": 100, "hit_in_cell_2": 100, "len_zero": 50}))
    d = INSIDE_DIMS
    Kd, god, _ = front_view(d, (15, 17), "z", surf=6.3)
    god = god + OFF_CENTRE["z"]
    t, w = plane_state(d, [0, 0, 1], 6.3)
    i, j, k = voxel_coords(d)
    t[(k == 1) & (i % 2 == 0)] = 3e38
    t[(k == 1) & (i % 2 == 1)] = -3e38
    out.append(case("neighbours of +-3e38", "the interpolation overflows: F not finite, the sample invalid", d, (t, w), Kd,
                    (15, 17), cam_at(god), ids_too=True, expect={"overflow_invalid": 100, "hit": 64}))
    # a weight at the threshold on isolated voxels of the layer k = 6: each is a single corner of the cells around it
    lone = (k == 6) & (i % 4 == 1) & (j % 4 == 2)
    for what, wv, exp, nev in (("exactly at the threshold", f32(0.9), {"weight_invalid": 8}, ()),
                               ("one ulp above the threshold", np.nextafter(f32(0.9), f32(2)), {"hit": 128}, ("weight_invalid",)),
                               ("NaN", f32(np.nan), {"weight_invalid": 8}, ())):
        t, w = plane_state(d, [0, 0, 1], 6.3)
        w[lone] = wv
        out.append(case(f"weight {what} on single corners", "w > weight_thresh", d, (t, w), Kd, (15, 17), cam_at(god),
                        ids_too=True, expect=exp, never=nev))
    t, w = plane_state(d, [0, 0, 1], 6.3)
    w[lone] = 0.0
    w[(k == 3) & (i % 3 == 0)] = -0.5
    out.append(case("thr negative", "zero and negative weights above a negative threshold", d, (t, w), Kd, (15, 17), cam_at(god),
                    thr=-1.0, ids_too=True, expect={"hit": 128}, never=("weight_invalid",), plane=(np.array([0.0, 0, 1]), 6.3)))
    out.append(case("thr = +inf", "no weight is above it", d, plane_state(d, [0, 0, 1], 6.3), Kd, (15, 17), cam_at(god),
                    thr=np.inf, expect={"weight_invalid": 200}, never=("hit",), miss=True))
    return out


def normal_cases():
    out = []
    d = LABEL_GRIDS[2]
    # a wide image over the whole x, y extent: hits within a voxel of the four side faces; planes half a voxel inside the
    # near and the far z face: a central-difference sample falls outside, the normal is (0, 0, 0), the depth is kept
    # (the march towards a plane near the far face starts, through near, 4.3 voxels before it: steps of 3.4 and then of one voxel put
    # the sample that sees F <= 0 inside the box on every ray)
    for what, z in (("low z face", 0.4), ("high z face", 10.4), ("middle", 6.3)):
        Kd, god, _ = front_view(d, (17, 33), "z", dist=60.0, surf=z, fill=(1.02, 1.04))
        god = god + np.array([0.0, -0.1, 0.0])           # the centre row off g_y = 9.5, a rounding boundary of the label voxel
        near = (60 + z - 4.3) * 0.0625 if z > 10 else 0.0
        exp = {"normal_zero_near_lo_x": 1, "normal_zero_near_hi_x": 1, "normal_zero_near_lo_y": 1, "normal_zero_near_hi_y": 1,
               "vox_lo_x": 1, "vox_hi_x": 1, "vox_lo_y": 1, "vox_hi_y": 1}
        if z < 1:
            exp.update(normal_zero_near_lo_z=100, vox_lo_z=1)
        elif z > 10:
            exp.update(normal_zero_near_hi_z=100)
        else:
            exp.update(normal_unit=100)
        out.append(case(f"hits beside the side faces, plane near the {what}", "a normal sample outside the box", d,
                        plane_state(d, [0, 0, 1], z), Kd, (17, 33), cam_at(god), near=near, ids_too=True, expect=exp,
                        plane=(np.array([0.0, 0, 1]), z)))
    Kd, god, _ = front_view(d, (17, 33), "z", dist=60.0, surf=10.8, fill=(1.02, 1.04))
    god = god + np.array([0.0, -0.1, 0.0])
    out.append(case("hits within half a voxel of the high z face", "label voxel beside hi_z", d, plane_state(d, [0, 0, 1], 10.8), Kd,
                    (17, 33), cam_at(god), near=(60 + 10.8 - 4.3) * 0.0625, ids_too=True, expect={"vox_hi_z": 100}, plane=(np.array([0.0, 0, 1]), 10.8)))
    # zero-weight voxels one layer behind the surface: the +1 sample of the normal lands in a cell that holds one
    Kd, god, _ = front_view(d, (15, 17), "z", surf=6.3)
    t, w = plane_state(d, [0, 0, 1], 6.3)
    i, j, k = voxel_coords(d)
    w[(k == 8) & (i % 4 == 1) & (j % 4 == 2)] = 0.0
    out.append(case("a normal sample in a zero-weight cell", "an invalid normal sample inside the box", d, (t, w), Kd, (15, 17),
                    cam_at(god), ids_too=True, expect={"normal_zero_interior": 8, "normal_unit": 64}))
    # F = 2 on the first two layers (a step of 8 voxels), then zero everywhere: the hit and its six neighbours all read 0
    const = layer_state(d, 2, [2.0, 2.0] + [0.0] * 10)
    out.append(case("constant F around the hit", "len == 0", d, const, Kd, (15, 17), cam_at(god), ids_too=True,
                    expect={"len_zero": 64}))
    # len not finite through values: +-3e38 two layers either side of the crossing; the first sample (near) is at g_z = 5.2,
    # where F = 0.6, the second lands among the -3e38; n_z is about -3e38 and its square overflows
    big = layer_state(d, 2, [3e38] * 5 + [1.0, -1.0] + [-3e38] * 5)
    out.append(case("len not finite", "n_i * n_i overflows", d, big, Kd, (15, 17), cam_at(god), near=(6 + 5.2) * 0.0625, ids_too=True,
                    expect={"len_not_finite": 64}))
    return out


def voxel_cases():
    out = []
    dims = LABEL_GRIDS[1]
    # go_x = 3.5 and gd_x == 0 on the centre column: g*_x + 0.5 == 4 exactly (the floorf tie) on the 17 rays of that column, 3 % of 17 x 33
    plane = (np.array([0.0, 0, 1]), 2.2)
    state = plane_state(dims, *plane)
    K, go, _ = front_view(dims, (17, 33), "z", surf=plane[1], fill=0.8, integer_centre=True)
    g = go.copy()
    g[0] = 3.5
    out.append(case("g*_x + 0.5 an exact integer", "the floorf tie of the label voxel", dims, state, K, (17, 33), cam_at(g),
                    ids_too=True, expect={"floor_tie_x": 17}, plane=plane))
    # a plane at g_z = 1.5 with a dyadic field and steps of exactly vs on the centre ray: g*_z + 0.5 == 2 exactly there; every
    # other ray lands within rounding of the tie, which is why the float64 label check does not apply
    t, w = plane_state(dims, [0, 0, 1], 1.5, scale=64.0)
    out.append(case("g*_z + 0.5 an exact integer", "the floorf tie of the label voxel", dims, (t, w), K, (17, 33), cam_at(go),
                    ids_too=True, expect={"floor_tie_z": 1, "hit": 64}, plane=(np.array([0.0, 0, 1]), 1.5), f64_labels=False))
    return out


def single_cases():
    base = (shape_cases() + axis_parallel_cases() + box_cases() + inside_and_singular_cases() + nonfinite_pose_cases()
            + march_cases() + value_cases() + normal_cases() + voxel_cases())
    out = list(base)
    for c in base:
        if c["name"] in NOT_REBASED:
            continue
        out.append(rebased(c, BASE_QUARTER, "quarter-turn base frame"))
        if c["plane"] is not None and c["tilt"]:
            out.append(rebased(c, BASE_TILT, "tilted base frame", keep_classes=False))
    names = [c["name"] for c in out]
    assert len(set(names)) == len(names)
    return out


# a base translation of order 1 is lost in a camera 1e6 m or 3e38 m away, and NaN / inf spread through the composition: these
# stay in the identity frame, where their classes are proved
NOT_REBASED = {"camera 1e6 m away", "translation of 3e38", "NaN in the rotation", "inf in the rotation", "NaN in the translation",
               "-inf in the translation"}


# ------------------------------------------------------------------------------------------------------------------------
# batch
# ------------------------------------------------------------------------------------------------------------------------
def member(dims, state, base, vs=VS, origin=ORIGIN, trunc=None):
    """A batch member: its grid, its state and its own base frame."""
    trunc = float(f32(vs) * f32(5)) if trunc is None else float(trunc)
    return dict(dims=tuple(dims), vs=float(vs), origin=np.asarray(origin, f32), trunc=trunc, tsdf=state[0], weight=state[1],
                base2world=np.asarray(base, f64).astype(f32))


BATCH_K = intrinsics(12.0, 12.0, 8.0, 7.0)
BATCH_HW = (15, 17)


def flat_member(dims, z, dist, base=np.eye(4), shift=(0.0, 0.0), vs=VS, trunc=None, scale=5.0, weight=2.0):
    """A member holding a plane square to z at g_z = z whose low z face is `dist` voxels in front of the camera at the
    world origin when base is the identity: origin = -vs * (centre + shift, -dist)."""
    origin = -f64(vs) * np.array([(dims[0] - 1) / 2 + shift[0], (dims[1] - 1) / 2 + shift[1], -dist])
    return member(dims, plane_state(dims, [0, 0, 1], z, scale=scale, weight=weight), base, vs=vs, origin=origin, trunc=trunc)


def batch_case(name, branch, members, *, cam2world=np.eye(4), near=0.0, far=6.0, thr=0.9, expect=None, miss=False):
    return dict(name=name, branch=branch, members=members, K=BATCH_K, hw=BATCH_HW, near=near, far=far, thr=thr,
                cam2world=np.asarray(cam2world, f32), expect=dict(expect or {}), miss=miss)


def batch_cases():
    """tsdf_batch_create takes members whose dim_x is a multiple of 4 only (tests/test_gpu_raycast_exact.py asserts the refusal of
    a 9 x 7 x 5 member), so the members' shapes are those of GRIDS with dim_x rounded to one."""
    out = []
    A = flat_member((8, 7, 5), 1.5, 6.0, scale=64.0)                 # dyadic field: t* == 7.5 * vs on rays that round alike
    A2 = flat_member((8, 7, 5), 1.5, 6.0, scale=64.0)
    C = flat_member((8, 7, 5), 2.3, 9.0, shift=(4.0, 2.0))          # farther, shifted: it shows beside A
    out.append(batch_case("twins", "an exact tie goes to the lower index", [A, A2], expect={"tie": 48, "member_0": 48}))
    out.append(batch_case("twins before a farther member", "tie, then a farther hit", [A, A2, C],
                          expect={"tie": 48, "member_0": 48, "member_2": 8}))
    out.append(batch_case("twins after a farther member", "a nearer pair placed after a farther member", [C, A, A2],
                          expect={"tie": 48, "member_1": 48, "member_0": 8}))
    out.append(batch_case("nearer after farther", "ts < best replaces the best", [C, A], expect={"member_1": 48, "member_0": 8,
                                                                                                 "replaced": 16}))
    out.append(batch_case("farther after nearer", "the box cull and ts < best keep the best", [A, C],
                          expect={"member_0": 48, "member_1": 8, "culled": 16}))
    # a member whose near face is at camera z = 7.5 * vs, the twins' t* : t_enter == best on the rays whose t* rounds to
    # exactly that, an ulp either side on others
    D = flat_member((8, 7, 5), 1.2, 7.5)
    out.append(batch_case("box entered at the best hit", "!(t_enter < best) at equality", [A, D],
                          expect={"t_enter_equals_best": 8, "member_0": 48}))
    Dm = flat_member((8, 7, 5), 1.2, float(np.nextafter(f32(7.5 * 0.0625), f32(0))) / 0.0625)
    out.append(batch_case("box entered an ulp before the best hit", "!(t_enter < best) one ulp below", [A, Dm],
                          expect={"t_enter_ulp_below_best": 8, "member_0": 48}))
    n_vox = 8 * 7 * 5
    E = dict(A, tsdf=np.ones(n_vox, f32), weight=np.zeros(n_vox, f32))
    G = dict(flat_member((8, 7, 5), 1.5, 6.0), origin=np.array([3e38, 0, 0], f32))        # go_x = -3e38 / vs = -inf
    out.append(batch_case("an empty member and one with go not finite between two that hit", "members that cannot hit",
                          [C, E, G, A], expect={"member_3": 48, "member_0": 8}))
    out.append(batch_case("one member", "n = 1", [A], expect={"member_0": 48}))
    # two to five members of different dims, vs and trunc, each in its own base frame; the camera is at a tilted world pose
    c2w = pose(rot([0.2, 1.0, -0.1], 0.4), [0.3, -0.2, 0.1])
    mixed = []
    for k, (dims, vs, z, dist, shift, tr) in enumerate([((8, 7, 5), 0.0625, 2.2, 8.0, (3.0, 0.0), 5.0),
                                                        ((16, 2, 3), 0.05, 1.1, 9.0, (-2.0, 2.0), 3.0),
                                                        ((4, 3, 17), 0.04, 8.0, 6.0, (0.0, -3.0), 6.0),
                                                        ((32, 20, 12), 0.03, 6.3, 30.0, (0.0, 0.0), 5.0),
                                                        ((4, 2, 2), 0.25, 0.5, 1.5, (0.0, 0.0), 5.0)]):
        rel = pose(rot([1.0, 0.3 * k, 0.2], 0.1 * k), [0.0, 0.0, 0.0])       # cam2base of this member
        mixed.append(flat_member(dims, z, dist, base=c2w @ np.linalg.inv(rel), shift=shift, vs=f32(vs),
                                 trunc=float(f32(vs) * f32(tr)), scale=tr))
    out.append(batch_case("five members in their own base frames", "dims, vs, trunc and base2world per member", mixed,
                          cam2world=c2w, expect={"members_seen_4": 1}))
    out.append(batch_case("two members in their own base frames", "dims, vs, trunc and base2world per member", mixed[3:0:-2],
                          cam2world=c2w, expect={"members_seen_2": 1}))
    return out
