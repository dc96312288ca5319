"""Every file the library writes for one small fused, coloured scene (tests/files_cases.py), byte for byte against
tests/files_spec.py built from the handle's own extraction and downloads, and against the oracle's writers: a handle over the
whole grid, one over z in [5, 12) (so the colour lookup subtracts a first slice), a group of three slabs and a handle nothing
was integrated into; with and without colour; and a device that takes no byte (/dev/full) on the writers that
tests/test_gpu_parity.py leaves out."""
import numpy as np
import pytest

import files_cases as fc
import files_spec as fs
from semantic_slam_amd import capi

pytestmark = pytest.mark.gpu

MESH_SAVERS = ("save_mesh_ply", "save_mesh_welded_ply")


def saved(tmp, fn, name):
    fn(str(tmp / name))
    return (tmp / name).read_bytes()


@pytest.fixture(scope="module")
def handles(cuda):
    """{name: Volume}: 'whole' and 'upper' fused from depth alone (colour not enabled yet), 'fresh' with nothing integrated."""
    vols = {"whole": capi.Volume(fc.config()), "upper": capi.Volume(fc.config(z_begin=fc.Z_CUT)), "fresh": capi.Volume(fc.config())}
    for name in ("whole", "upper"):
        for pose, depth, _ in fc.frames():
            vols[name].integrate(depth, pose)
    yield vols
    for v in vols.values():
        v.close()


@pytest.fixture(scope="module")
def plain_files(handles, tmp_path_factory):
    """The files of the handles before colour_enable, and what the spec says they are: {handle: {saver: (bytes, spec's bytes)}}."""
    tmp = tmp_path_factory.mktemp("plain")
    out = {}
    for name, v in handles.items():
        tri, xyz, (t, _) = v.extract_mesh(), v.extract_surface(), v.download()
        nz = v.cfg.z_end - v.cfg.z_begin
        out[name] = {"save_mesh_ply": (saved(tmp, v.save_mesh_ply, name + ".soup.ply"), fs.soup_ply(tri)),
                     "save_mesh_welded_ply": (saved(tmp, v.save_mesh_welded_ply, name + ".welded.ply"), fs.welded_ply(tri)),
                     "save_ply": (saved(tmp, v.save_ply, name + ".points.ply"), fs.points_ply(xyz)),
                     "save_bin": (saved(tmp, v.save_bin, name + ".bin"),
                                  fs.bin_header(fc.DIMS[:2], nz, fc.ORIGIN, fc.VS, v.cfg.trunc_margin) + t.tobytes()),
                     "n": (len(tri), len(xyz))}
    return out


@pytest.fixture(scope="module")
def coloured(handles, plain_files):
    """'whole' and 'upper' again, reset, colour enabled and the same frames given with their images (after plain_files)."""
    for name in ("whole", "upper"):
        v = handles[name]
        v.reset()
        v.colour_enable()
        for pose, depth, rgb in fc.frames():
            v.integrate_rgbd(depth, rgb, pose)
    return {name: handles[name] for name in ("whole", "upper")}


@pytest.mark.parametrize("name", ["whole", "upper", "fresh"])
@pytest.mark.parametrize("saver", MESH_SAVERS + ("save_ply", "save_bin"))
def test_files_without_colour_match_the_spec(plain_files, name, saver):
    got, want = plain_files[name][saver]
    assert got == want
    n_tri, n_pts = plain_files[name]["n"]
    if name == "fresh":
        assert (n_tri, n_pts) == (0, 0)
        if saver != "save_bin":    # 0 vertices, 0 faces: a header only
            assert got.endswith(b"end_header\n") and b"element vertex 0\n" in got
            assert b"element face 0\n" in got or saver == "save_ply"
    else:
        assert n_tri > 300 and n_pts > 300
    if saver != "save_bin":
        assert b"red" not in got[:got.index(b"end_header\n")]


def test_whole_grid_files_match_the_oracle_writers(plain_files, oracle, tmp_path):
    t, w, _ = fc.oracle_state()
    cfg = fc.config()
    oracle.save_ply(str(tmp_path / "o.ply"), np.array(t), np.array(w), fc.DIMS, fc.VS, fc.ORIGIN)
    oracle.save_bin(str(tmp_path / "o.bin"), np.array(t), fc.DIMS, fc.ORIGIN, fc.VS, cfg.trunc_margin)
    assert plain_files["whole"]["save_ply"][0] == (tmp_path / "o.ply").read_bytes()
    assert plain_files["whole"]["save_bin"][0] == (tmp_path / "o.bin").read_bytes()


@pytest.mark.parametrize("name", ["whole", "upper"])
def test_coloured_mesh_files_match_the_spec(coloured, plain_files, tmp_path, name):
    v = coloured[name]
    tri, colour = v.extract_mesh(), v.download_colour()
    g = fs.grid_of(v.cfg)
    assert len(tri) == plain_files[name]["n"][0] and len(np.unique(colour)) > 100
    soup, welded = saved(tmp_path, v.save_mesh_ply, "soup.ply"), saved(tmp_path, v.save_mesh_welded_ply, "welded.ply")
    for got in (soup, welded):
        assert b"property uchar red\nproperty uchar green\nproperty uchar blue\n" in got[:got.index(b"end_header\n")]
    assert soup == fs.soup_ply(tri, g, colour)
    assert welded == fs.welded_ply(tri, g, colour)
    if name == "upper":      # the lookups would land elsewhere without the slab's first slice
        verts = fs.weld(tri)[0]
        assert np.count_nonzero(fs.nearest_voxel(g, verts) != fs.nearest_voxel(dict(g, z_begin=0, z_end=g["z_end"] - g["z_begin"]), verts)) > 100


@pytest.fixture(scope="module")
def group(cuda):
    with capi.Group(fc.config(), [0, 0, 0]) as g:
        for pose, depth, _ in fc.frames():
            g.integrate(depth, pose)
        yield g


@pytest.mark.parametrize("saver", ["save_ply", "save_mesh_ply", "save_bin"])
def test_group_files_equal_the_whole_handle_s(group, plain_files, tmp_path, saver):
    assert saved(tmp_path, getattr(group, saver), "g") == plain_files["whole"][saver][0]


def test_a_full_disk_is_reported_and_changes_nothing(coloured, group):
    t_ref, w_ref, _ = fc.oracle_state()
    for name, v in coloured.items():
        before = v.download()
        for saver in MESH_SAVERS:
            with pytest.raises(capi.TsdfError) as e:
                getattr(v, saver)("/dev/full")
            assert "short write" in str(e.value) or "cannot" in str(e.value), (name, saver)
        after = v.download()
        assert all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(before, after))
    for saver in ("save_ply", "save_mesh_ply", "save_bin"):
        with pytest.raises(capi.TsdfError) as e:
            getattr(group, saver)("/dev/full")
        assert "short write" in str(e.value) or "cannot" in str(e.value), saver
    t, w = group.download()
    assert np.array_equal(t.view(np.uint32), t_ref.view(np.uint32)) and np.array_equal(w, w_ref)
