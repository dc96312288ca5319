"""The file formats of semantic_slam_amd/csrc/mesh_files.h restated in NumPy (test infrastructure), byte for byte: the points
.ply, the .bin header, the mesh .ply as a triangle soup and welded with normals, and the colour a vertex takes from its nearest
voxel.  Every operation is an IEEE basic operation or sqrt in the precision the header uses, so the bytes are specified
exactly: quotients in float32, rounding half away from zero, normals summed in float64 in face order.

A grid is a dict: dims (x, y, z of the whole grid), z_begin, z_end (the slab the colour array covers), origin [3], voxel_size.
"""
import numpy as np

f32 = np.float32


def grid(dims, origin, voxel_size, z_begin=0, z_end=None):
    return {"dims": tuple(int(d) for d in dims), "z_begin": int(z_begin), "z_end": int(dims[2] if z_end is None else z_end),
            "origin": np.asarray(origin, f32), "voxel_size": f32(voxel_size)}


def grid_of(cfg):
    """The grid of a capi.TsdfConfig."""
    return grid((cfg.dim_x, cfg.dim_y, cfg.dim_z), [cfg.origin[i] for i in range(3)], cfg.voxel_size, cfg.z_begin, cfg.z_end)


# ---- surface points ------------------------------------------------------------------------------------------------------
def points_ply(xyz):
    xyz = np.ascontiguousarray(xyz, f32).reshape(-1, 3)
    head = (f"ply\nformat binary_little_endian 1.0\nelement vertex {len(xyz)}\n"
            "property float x\nproperty float y\nproperty float z\nend_header\n")
    return head.encode() + xyz.tobytes()


# ---- .bin ------------------------------------------------------------------------------------------------------------------
def bin_header(dims_xy, nz, origin, voxel_size, trunc):
    """8 float32: the file's dims, origin, voxel size, truncation margin; the TSDF values follow."""
    return np.array([dims_xy[0], dims_xy[1], nz, origin[0], origin[1], origin[2], voxel_size, trunc], f32).tobytes()


# ---- vertex colour ---------------------------------------------------------------------------------------------------------
def lround(q):
    """C's lround of float32 values: floor(|q| + 0.5) with q's sign (the sum is exact in float64)."""
    q = np.asarray(q, f32).astype(np.float64)
    return (np.sign(q) * np.floor(np.abs(q) + 0.5)).astype(np.int64)


def nearest_voxel(g, xyz):
    """Index into the slab's arrays (x fastest) of the voxel nearest to every point: the float32 quotient per axis, rounded,
    the slab's first slice subtracted from z, clamped into the slab."""
    xyz = np.asarray(xyz, f32).reshape(-1, 3)
    q = (xyz - g["origin"][None, :]) / g["voxel_size"]
    assert q.dtype == f32
    i = lround(q)
    dx, dy, _ = g["dims"]
    ix = np.clip(i[:, 0], 0, dx - 1)
    iy = np.clip(i[:, 1], 0, dy - 1)
    iz = np.clip(i[:, 2] - g["z_begin"], 0, g["z_end"] - g["z_begin"] - 1)
    return (iz * dy + iy) * dx + ix


def vertex_rgb(g, colour, xyz):
    """uint8 [n, 3]: r, g, b of the nearest voxel's packed 0x00BBGGRR."""
    q = np.asarray(colour, np.uint32).ravel()[nearest_voxel(g, xyz)]
    return np.stack([q & 255, (q >> 8) & 255, (q >> 16) & 255], axis=-1).astype(np.uint8)


# ---- meshes ----------------------------------------------------------------------------------------------------------------
def _records(floats, rgb):
    """One record per vertex: the float32 columns, then the 3 colour bytes when there are any."""
    floats = np.ascontiguousarray(floats, f32)
    rec = floats.view(np.uint8).reshape(len(floats), 4 * floats.shape[1])
    if rgb is not None:
        rec = np.concatenate([rec, np.asarray(rgb, np.uint8).reshape(len(floats), 3)], axis=1)
    return rec.tobytes()


def _faces(idx):
    idx = np.ascontiguousarray(idx, "<i4").reshape(-1, 3)
    rec = np.empty((len(idx), 13), np.uint8)
    rec[:, 0] = 3
    rec[:, 1:] = idx.view(np.uint8).reshape(len(idx), 12)
    return rec.tobytes()


def soup_ply(tri, g=None, colour=None):
    """n triangles, three vertices each, faces (3k, 3k + 1, 3k + 2); with a colour array every vertex carries its rgb."""
    tri = np.ascontiguousarray(tri, f32).reshape(-1, 3, 3)
    n = len(tri)
    head = f"ply\nformat binary_little_endian 1.0\nelement vertex {3 * n}\nproperty float x\nproperty float y\nproperty float z\n"
    if colour is not None:
        head += "property uchar red\nproperty uchar green\nproperty uchar blue\n"
    head += f"element face {n}\nproperty list uchar int vertex_indices\nend_header\n"
    verts = tri.reshape(-1, 3)
    rgb = vertex_rgb(g, colour, verts) if colour is not None else None
    return head.encode() + _records(verts, rgb) + _faces(np.arange(3 * n))


def weld(tri):
    """(verts [nv, 3] float32, faces [n, 3] int32, normals [nv, 3] float32): vertices distinct by their coordinates' bits
    (+0 and -0 differ), numbered at first appearance; a normal is the float64 sum, in face order, of the cross products
    (b - a) x (c - a) of the vertex's faces, normalised and rounded to float32, or (0, 0, 0) where the sum is."""
    tri = np.ascontiguousarray(tri, f32).reshape(-1, 3, 3)
    n = len(tri)
    if n == 0:
        return np.zeros((0, 3), f32), np.zeros((0, 3), np.int32), np.zeros((0, 3), f32)
    flat = tri.reshape(-1, 3)
    _, first, inverse = np.unique(flat.view(np.uint32).reshape(-1, 3), axis=0, return_index=True, return_inverse=True)
    inverse = np.asarray(inverse).reshape(-1)
    order = np.argsort(first, kind="stable")               # np.unique sorts by value: renumber by first appearance
    rank = np.empty(len(order), np.int64)
    rank[order] = np.arange(len(order))
    faces = rank[inverse].astype(np.int32).reshape(n, 3)
    verts = flat[first[order]]
    d = tri.astype(np.float64)
    u, w = d[:, 1] - d[:, 0], d[:, 2] - d[:, 0]
    fn = np.stack([u[:, 1] * w[:, 2] - u[:, 2] * w[:, 1], u[:, 2] * w[:, 0] - u[:, 0] * w[:, 2], u[:, 0] * w[:, 1] - u[:, 1] * w[:, 0]], axis=-1)
    acc = np.zeros((len(verts), 3), np.float64)
    np.add.at(acc, faces.reshape(-1), np.repeat(fn, 3, axis=0))
    length = np.sqrt((acc[:, 0] * acc[:, 0] + acc[:, 1] * acc[:, 1]) + acc[:, 2] * acc[:, 2])
    with np.errstate(invalid="ignore", divide="ignore"):
        normals = np.where(length[:, None] > 0, acc / length[:, None], 0.0).astype(f32)
    return verts, faces, normals


def welded_ply(tri, g=None, colour=None):
    verts, faces, normals = weld(tri)
    head = (f"ply\nformat binary_little_endian 1.0\nelement vertex {len(verts)}\nproperty float x\nproperty float y\n"
            "property float z\nproperty float nx\nproperty float ny\nproperty float nz\n")
    if colour is not None:
        head += "property uchar red\nproperty uchar green\nproperty uchar blue\n"
    head += f"element face {len(faces)}\nproperty list uchar int vertex_index\nend_header\n"
    rgb = vertex_rgb(g, colour, verts) if colour is not None else None
    return head.encode() + _records(np.concatenate([verts, normals], axis=1), rgb) + _faces(faces)
