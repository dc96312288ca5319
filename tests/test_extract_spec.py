"""An independent float64 NumPy statement of the extraction and mask-composition rules, written from the comments that
define them (semantic_slam_amd/csrc/tsdf_extract.hip.h: the header of the file for surface points, the comment above
CrossingGrid for zero crossings, the marching-tetrahedra comment with its kTet table for the mesh;
tsdf_labels.hip.h above ComposeParams for compose_labels), compared with the C oracle on small random grids seeded with
the value edges the kernels' sign and weight tests meet: NaN, +-inf, -0.0 and 0.0 TSDF values; weights at the threshold,
one ulp above it, NaN and negative; thresholds 0, 0.9, 1, 2.5, -1 and NaN.  The GPU suite compares the kernels with the
oracle bit for bit, so this pins both to the written rule.

Readings of the comments that the text leaves open, stated once here:
  * "opposite sign" of the crossing rule is the mesh rule's inside test, tsdf < 0: -0.0 and NaN count as outside;
  * a weight test "weight > thr" is false for a NaN weight or a NaN threshold;
  * "the inside corner" of the winding rule is the tetrahedron's first inside corner in kTet order.
"""
import numpy as np
import pytest

from fuzz_cases import THRESHOLDS, edge_values

f32 = np.float32
# the six tetrahedra around the cube diagonal 0-7 (corner c = dx + 2 dy + 4 dz), kTet of tsdf_extract.hip.h
TETS = [(0, 1, 3, 7), (0, 3, 2, 7), (0, 2, 6, 7), (0, 6, 4, 7), (0, 4, 5, 7), (0, 5, 1, 7)]


def above(w, thr):
    with np.errstate(invalid="ignore"):
        return np.asarray(w, np.float64) > np.float64(f32(thr))


def inside(t):
    with np.errstate(invalid="ignore"):
        return np.asarray(t, np.float64) < 0.0


def spec_surface(t, w, dims, vs, origin, thr):
    """Voxel i is kept when |tsdf[i]| != 0 and weight[i] > thr; point = origin + index * voxel_size, grid order."""
    dx, dy, dz = dims
    with np.errstate(invalid="ignore"):
        keep = (np.abs(t.astype(np.float64)) != 0.0) & above(w, thr)
    idx = np.nonzero(keep)[0]
    z, rem = np.divmod(idx, dx * dy)
    y, x = np.divmod(rem, dx)
    o = np.asarray(origin, np.float64)
    v = np.float64(f32(vs))
    return np.stack([o[0] + x * v, o[1] + y * v, o[2] + z * v], axis=1).reshape(-1, 3), idx


def spec_crossings(t, w, dims_xy, z_begin, z_end, vs, origin, thr, halo=None):
    """For voxel v and axis a with neighbour n = v + e_a inside the slab (or, for the top slice's +z edge, in the halo):
    both weights > thr and the signs differ -> p(v) + t(v) / (t(v) - t(n)) * vs * e_a; voxels in grid order, then x, y, z."""
    dx, dy = dims_xy
    nz = z_end - z_begin
    T = t.astype(np.float64).reshape(nz, dy, dx)
    W = w.reshape(nz, dy, dx)
    if halo is not None:
        T = np.concatenate([T, halo[0].astype(np.float64).reshape(1, dy, dx)])
        W = np.concatenate([W, halo[1].reshape(1, dy, dx)])
    ok = above(W, thr)
    neg = inside(T)
    o = np.asarray(origin, np.float64)
    v = np.float64(f32(vs))
    items = []
    for z in range(nz):
        for y in range(dy):
            for x in range(dx):
                if not ok[z, y, x]:
                    continue
                p = np.array([o[0] + x * v, o[1] + y * v, o[2] + (z_begin + z) * v])
                for a, (nx, ny, nzz) in enumerate(((x + 1, y, z), (x, y + 1, z), (x, y, z + 1))):
                    if nx >= dx or ny >= dy or nzz >= T.shape[0]:
                        continue
                    if not ok[nzz, ny, nx] or neg[z, y, x] == neg[nzz, ny, nx]:
                        continue
                    t0, t1 = T[z, y, x], T[nzz, ny, nx]
                    with np.errstate(invalid="ignore", divide="ignore"):
                        s = t0 / (t0 - t1)
                    q = p.copy()
                    q[a] += s * v
                    items.append(((z, y, x, a), q))
    return [k for k, _ in items], np.array([q for _, q in items]).reshape(-1, 3)


def spec_mesh(t, w, dims_xy, z_begin, z_end, vs, origin, thr, halo=None):
    """Per cube (base voxel in grid order) whose 8 corners have weight > thr, per tetrahedron of TETS: the edge points of
    the tetrahedron (1 or 3 corners inside -> the 3 edges of the odd corner, 2 -> the 4 edges between the inside and the
    outside pair), its first inside corner, and the number of triangles it yields."""
    dx, dy = dims_xy
    nz = z_end - z_begin
    T = t.astype(np.float64).reshape(nz, dy, dx)
    W = w.reshape(nz, dy, dx)
    if halo is not None:
        T = np.concatenate([T, halo[0].astype(np.float64).reshape(1, dy, dx)])
        W = np.concatenate([W, halo[1].reshape(1, dy, dx)])
    ok = above(W, thr)
    o = np.asarray(origin, np.float64)
    v = np.float64(f32(vs))
    tets = []
    for z in range(T.shape[0] - 1):
        for y in range(dy - 1):
            for x in range(dx - 1):
                cs = [(x + (c & 1), y + ((c >> 1) & 1), z + (c >> 2)) for c in range(8)]
                if not all(ok[cz, cy, cx] for cx, cy, cz in cs):
                    continue
                tv = [T[cz, cy, cx] for cx, cy, cz in cs]
                p = [np.array([o[0] + cx * v, o[1] + cy * v, o[2] + (z_begin + cz) * v]) for cx, cy, cz in cs]
                for k, tet in enumerate(TETS):
                    ins = [bool(inside(tv[c])) for c in tet]
                    n_in = sum(ins)
                    if n_in in (0, 4):
                        continue

                    def edge(i, j):
                        i, j = min(i, j), max(i, j)       # lower corner first
                        with np.errstate(invalid="ignore", divide="ignore"):
                            s = tv[i] / (tv[i] - tv[j])
                            return p[i] + s * (p[j] - p[i])

                    if n_in in (1, 3):
                        odd = [c for c, f in zip(tet, ins) if f == (n_in == 1)][0]
                        pts = [edge(odd, c) for c in tet if c != odd]
                    else:
                        a_in = [c for c, f in zip(tet, ins) if f]
                        a_out = [c for c, f in zip(tet, ins) if not f]
                        pts = [edge(a, b) for a in a_in for b in a_out]
                    q = p[[c for c, f in zip(tet, ins) if f][0]]
                    tets.append(((z, y, x, k), np.array(pts), q, 2 if n_in == 2 else 1))
    return tets


def ulp_tol(*arrays):
    m = max([float(np.max(np.abs(a[np.isfinite(a)]), initial=0.0)) for a in arrays] + [1.0])
    return 4.0 * float(np.spacing(f32(m)))


def assert_coords(got, want, tol, what):
    got = np.asarray(got, np.float64)
    assert got.shape == want.shape, what
    assert np.array_equal(np.isnan(got), np.isnan(want)), f"{what}: NaN positions differ"
    fin = ~np.isnan(want)
    assert np.array_equal(np.isinf(got[fin]), np.isinf(want[fin])), f"{what}: infinities differ"
    diff = np.abs(np.where(np.isfinite(want), got - want, 0.0))
    assert float(diff.max(initial=0.0)) <= tol, f"{what}: {float(diff.max())} > {tol}"


def random_grid(seed):
    rng = np.random.default_rng(7000 + seed)
    dims = (int(rng.integers(1, 9)), int(rng.integers(1, 7)), int(rng.integers(1, 6)))
    thr = THRESHOLDS[seed % len(THRESHOLDS)]
    t, w = edge_values(rng, dims[0] * dims[1] * dims[2], thr)
    vs = float(rng.choice([0.004, 0.01, 0.05, 0.3]))
    origin = rng.uniform(-2.0, 2.0, 3).astype(f32)
    return rng, dims, thr, t, w, vs, origin


SEEDS = range(36)


@pytest.mark.parametrize("seed", SEEDS)
def test_surface_points_follow_the_written_rule(oracle, seed):
    _, dims, thr, t, w, vs, origin = random_grid(seed)
    want, _ = spec_surface(t, w, dims, vs, origin, thr)
    got = oracle.surface_points(t, w, dims, vs, origin, weight_thresh=thr)
    assert_coords(got, want, ulp_tol(want), f"seed {seed}")


@pytest.mark.parametrize("seed", SEEDS)
def test_crossings_follow_the_written_rule(oracle, seed):
    rng, dims, thr, t, w, vs, origin = random_grid(seed)
    dx, dy, dz = dims
    keys, want = spec_crossings(t, w, (dx, dy), 0, dz, vs, origin, thr)
    got = oracle.zero_crossings(t, w, (dx, dy), 0, dz, vs, origin, weight_thresh=thr)
    assert_coords(got, want, ulp_tol(want), f"seed {seed}")
    # a slab [z0, z1) with the next slice as its halo, and without: the same items of the whole list, then fewer
    if dz >= 2:
        z0 = int(rng.integers(0, dz - 1))
        z1 = int(rng.integers(z0 + 1, dz))
        s = dx * dy
        part = (t[z0 * s:z1 * s], w[z0 * s:z1 * s])
        halo = (t[z1 * s:(z1 + 1) * s], w[z1 * s:(z1 + 1) * s])
        k2, w2 = spec_crossings(*part, (dx, dy), z0, z1, vs, origin, thr, halo=halo)
        assert k2 == [(z - z0, y, x, a) for z, y, x, a in keys if z0 <= z < z1]
        g2 = oracle.zero_crossings(*part, (dx, dy), z0, z1, vs, origin, halo=halo, weight_thresh=thr)
        assert_coords(g2, w2, ulp_tol(w2), f"seed {seed} slab {z0}:{z1}")
        k3, w3 = spec_crossings(*part, (dx, dy), z0, z1, vs, origin, thr)
        assert k3 == [k for k in k2 if not (k[0] == z1 - z0 - 1 and k[3] == 2)]
        g3 = oracle.zero_crossings(*part, (dx, dy), z0, z1, vs, origin, weight_thresh=thr)
        assert_coords(g3, w3, ulp_tol(w3), f"seed {seed} slab {z0}:{z1} without halo")


def check_mesh(got, tets, what):
    """got: the oracle's [n, 3, 3] list.  Walk the spec's tetrahedra in order: each owns the next 1 or 2 triangles, whose
    vertices are its edge points (the two triangles of a quad share one of its diagonals), wound away from its first
    inside corner."""
    got = np.asarray(got, np.float64)
    assert len(got) == sum(n for *_, n in tets), f"{what}: {len(got)} triangles, the rule gives {sum(n for *_, n in tets)}"
    tol = ulp_tol(got.reshape(-1, 3), *[p for _, p, _, _ in tets])
    pos = 0
    for key, pts, q, n in tets:
        tris = got[pos:pos + n]
        pos += n
        used = set()
        order = []              # per triangle: the edge point each vertex is, where that is unambiguous
        for tri in tris:
            ids = []
            for vtx in tri:
                d = np.where(np.isnan(pts) & np.isnan(vtx), 0.0, np.abs(pts - vtx))
                match = [i for i in range(len(pts)) if np.all(d[i] <= tol)]
                assert match, f"{what}: tetrahedron {key}: vertex {vtx} is none of its edge points {pts}"
                used.update(match)
                ids.append(match[0] if len(match) == 1 else None)
            order.append(ids)
        assert len(used) == len(pts), f"{what}: tetrahedron {key}: triangles do not cover its edge points"
        if n == 2:      # a quad (edges a_in0-a_out0, a_in0-a_out1, a_in1-a_out0, a_in1-a_out1): sides are 0-1, 1-3, 3-2, 2-0
            distinct = all(np.abs(pts[i] - pts[j]).max() > tol for i in range(4) for j in range(i))
            if np.isfinite(pts).all() and distinct:
                shared = [i for i in range(4) if any(np.all(np.abs(tris[0][a] - pts[i]) <= tol) for a in range(3)) and
                          any(np.all(np.abs(tris[1][a] - pts[i]) <= tol) for a in range(3))]
                assert sorted(shared) in ([0, 3], [1, 2]), f"{what}: tetrahedron {key}: the two triangles share {shared}"
        for ids in order:       # winding, from the float64 edge points so that fp32 rounding cannot flip it
            if None in ids or not np.isfinite(pts[ids]).all():
                continue
            tri = pts[ids]
            nrm = np.cross(tri[1] - tri[0], tri[2] - tri[0])
            d = float(nrm @ (tri[0] - q))
            scale = float(np.linalg.norm(nrm)) * float(np.linalg.norm(tri[0] - q))
            if abs(d) > 1e-9 * scale:
                assert d > 0, f"{what}: tetrahedron {key}: triangle wound towards its inside corner"


@pytest.mark.parametrize("seed", SEEDS)
def test_mesh_follows_the_written_rule(oracle, seed):
    rng, dims, thr, t, w, vs, origin = random_grid(seed)
    dx, dy, dz = dims
    tets = spec_mesh(t, w, (dx, dy), 0, dz, vs, origin, thr)
    got = oracle.mesh_triangles(t, w, (dx, dy), 0, dz, vs, origin, weight_thresh=thr)
    check_mesh(got, tets, f"seed {seed}")
    if dz >= 2:
        z0 = int(rng.integers(0, dz - 1))
        z1 = int(rng.integers(z0 + 1, dz))
        s = dx * dy
        part = (t[z0 * s:z1 * s], w[z0 * s:z1 * s])
        halo = (t[z1 * s:(z1 + 1) * s], w[z1 * s:(z1 + 1) * s])
        t2 = spec_mesh(*part, (dx, dy), z0, z1, vs, origin, thr, halo=halo)
        assert [k for k, *_ in t2] == [(z - z0, y, x, k) for (z, y, x, k), *_ in tets if z0 <= z < z1]
        check_mesh(oracle.mesh_triangles(*part, (dx, dy), z0, z1, vs, origin, halo=halo, weight_thresh=thr), t2,
                   f"seed {seed} slab {z0}:{z1}")


def test_mesh_rule_meets_every_case():
    """The random grids above reach both branches of the rule (one triangle, two triangles) and NaN vertices."""
    n_by = {1: 0, 2: 0}
    nan_tets = 0
    for seed in SEEDS:
        _, dims, thr, t, w, vs, origin = random_grid(seed)
        for key, pts, q, n in spec_mesh(t, w, dims[:2], 0, dims[2], vs, origin, thr):
            nan_tets += int(np.isnan(pts).any())
            n_by[n] += 1
    assert n_by[1] > 20 and n_by[2] > 20 and nan_tets > 5, (n_by, nan_tets)


def test_crossing_rule_meets_the_value_edges():
    """Crossings with a NaN end, with -0.0 next to a negative value and with an infinite end exist in the random grids,
    and the weight test rejects the threshold itself while it accepts the next float up."""
    nan_pts = inf_ends = zero_ends = 0
    for seed in SEEDS:
        _, dims, thr, t, w, vs, origin = random_grid(seed)
        keys, pts = spec_crossings(t, w, dims[:2], 0, dims[2], vs, origin, thr)
        nan_pts += int(np.isnan(pts).any(axis=1).sum())
        T = t.reshape(dims[2], dims[1], dims[0])
        for z, y, x, a in keys:
            nb = T[z + (a == 2), y + (a == 1), x + (a == 0)]
            ends = (T[z, y, x], nb)
            inf_ends += int(any(np.isinf(e) for e in ends))
            zero_ends += int(any(e == 0 for e in ends))
    assert nan_pts > 5 and inf_ends > 5 and zero_ends > 5, (nan_pts, inf_ends, zero_ends)
    thr = f32(0.9)
    assert not above(np.array([thr]), thr)[0] and above(np.array([np.nextafter(thr, f32(2))]), thr)[0]


@pytest.mark.parametrize("seed", range(8))
def test_compose_labels_follows_the_written_rule(oracle, seed):
    """Per pixel the covering instance with the highest score wins, the lower index on ties; uncovered pixels get 0 / 0."""
    rng = np.random.default_rng(8000 + seed)
    k, h, w = int(rng.integers(1, 9)), int(rng.integers(1, 20)), int(rng.integers(1, 24))
    masks = (rng.uniform(0, 1, (k, h, w)) < 0.4).astype(np.uint8) * 255
    labels = rng.integers(1, 81, k).astype(np.uint16)
    scores = rng.choice(np.array([0.5, 0.75, 0.9, -0.25, 0.0], f32), k)   # ties and non-positive scores on purpose
    lab, sc = oracle.compose_labels(masks, labels, scores)
    want_l = np.zeros((h, w), np.uint16)
    want_s = np.zeros((h, w), f32)
    for yy in range(h):
        for xx in range(w):
            cover = [m for m in range(k) if masks[m, yy, xx]]
            if cover:
                best = max(cover, key=lambda m: (np.float64(scores[m]), -m))
                want_l[yy, xx], want_s[yy, xx] = labels[best], scores[best]
    assert np.array_equal(lab, want_l), f"seed {seed}"
    assert np.array_equal(sc.view(np.uint32), want_s.view(np.uint32)), f"seed {seed}"
