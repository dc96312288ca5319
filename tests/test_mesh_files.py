"""The file formats without a device: semantic_slam_amd/csrc/mesh_files.h behind tests/mesh_files_check.cpp, a stand-alone
program built with AddressSanitizer and UndefinedBehaviorSanitizer (every finding fatal) and run as a child process, against
tests/files_spec.py byte for byte: the points .ply, the soup and the welded mesh .ply with and without colour, the .bin header
and the nearest voxel of every vertex; and the two failure codes of every writer."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import files_cases as fc
import files_spec as fs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAGS = ["-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
CANNOT_OPEN, SHORT_WRITE = 1, 2
TRUNC = np.float32(0.15)


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    assert shutil.which("g++"), "the format check needs g++"
    exe = tmp_path_factory.mktemp("mesh_files") / "mesh_files_check"
    subprocess.check_call(["g++", *FLAGS, "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "semantic_slam_amd", "csrc"),
                           "-o", str(exe), os.path.join(ROOT, "tests", "mesh_files_check.cpp")])
    return str(exe)


def run(program, tmp_path, g, tri, colour, extra=()):
    """The program's files for one input, {name: bytes}, and its standard output."""
    tri = np.ascontiguousarray(tri, np.float32).reshape(-1, 3, 3)
    inp, out = tmp_path / "input.bin", tmp_path / "out"
    out.mkdir()
    with open(inp, "wb") as f:
        f.write(np.array([*g["dims"], g["z_begin"], g["z_end"], len(tri), colour is not None], np.int32).tobytes())
        f.write(np.array([*g["origin"], g["voxel_size"], TRUNC], np.float32).tobytes())
        f.write(tri.tobytes())
        if colour is not None:
            f.write(np.ascontiguousarray(colour, np.uint32).tobytes())
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    p = subprocess.run([program, str(inp), str(out), *extra], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert p.returncode == 0 and not p.stderr, f"rc {p.returncode}\n{p.stderr.decode()[-4000:]}"
    return {q.name: q.read_bytes() for q in out.iterdir()}, p.stdout.decode()


def check(files, g, tri, colour):
    tri = np.ascontiguousarray(tri, np.float32).reshape(-1, 3, 3)
    want = {"points.ply": fs.points_ply(tri.reshape(-1, 3)), "soup.ply": fs.soup_ply(tri), "welded.ply": fs.welded_ply(tri),
            "header.bin": fs.bin_header(g["dims"][:2], g["z_end"] - g["z_begin"], g["origin"], g["voxel_size"], TRUNC),
            "nearest.i64": fs.nearest_voxel(g, tri.reshape(-1, 3)).astype(np.int64).tobytes()}
    if colour is not None:
        want.update({"soup_rgb.ply": fs.soup_ply(tri, g, colour), "welded_rgb.ply": fs.welded_ply(tri, g, colour),
                     "rgb.u8": fs.vertex_rgb(g, colour, tri.reshape(-1, 3)).tobytes()})
    assert sorted(files) == sorted(want)
    for name in want:
        assert files[name] == want[name], f"{name}: {len(files[name])} bytes written, {len(want[name])} specified"


@pytest.mark.parametrize("z_begin", [0, fc.Z_CUT])
def test_fused_scene_matches_the_spec(program, tmp_path, z_begin):
    tri, colour = fc.oracle_mesh(z_begin)
    g = fs.grid(fc.DIMS, fc.ORIGIN, fc.VS, z_begin)
    verts, _, normals = fs.weld(tri)
    if z_begin == 0:       # the input is what it is meant to be: a real mesh, shared vertices, many colours, nothing clamped or tied
        rgb = fs.vertex_rgb(g, colour, verts)
        assert (len(tri), len(verts), len(np.unique(rgb, axis=0))) == (1600, 854, 224)
        q = ((verts - g["origin"]) / g["voxel_size"]).astype(np.float64)
        assert np.all(q - np.floor(q) != 0.5), "a vertex on a rounding tie"
        i = fs.lround(q)
        assert np.all(i >= 0) and np.all(i < np.array(fc.DIMS)), "a clamped vertex"
    else:                  # the slab's first slice is subtracted: without the term the lookups land 5 slices up or are clamped
        up = dict(g, z_begin=0, z_end=fc.DIMS[2] - z_begin)
        assert len(tri) > 300 and np.count_nonzero(fs.nearest_voxel(g, verts) != fs.nearest_voxel(up, verts)) > 100
    assert np.all(np.abs(np.linalg.norm(normals.astype(np.float64), axis=1) - 1.0) < 1e-6)
    files, _ = run(program, tmp_path, g, tri, colour)
    check(files, g, tri, colour)
    assert b"property uchar red" in files["soup_rgb.ply"] and b"property uchar red" not in files["soup.ply"]


def test_an_empty_mesh_is_a_header(program, tmp_path):
    g = fs.grid(fc.DIMS, fc.ORIGIN, fc.VS)
    colour = np.zeros(int(np.prod(fc.DIMS)), np.uint32)
    files, _ = run(program, tmp_path, g, np.zeros((0, 3, 3), np.float32), colour)
    check(files, g, np.zeros((0, 3, 3), np.float32), colour)
    for name in ("points.ply", "soup.ply", "soup_rgb.ply", "welded.ply", "welded_rgb.ply"):
        assert files[name].endswith(b"end_header\n") and b"element vertex 0\n" in files[name]
    assert b"element face 0\n" in files["welded_rgb.ply"] and b"property uchar red" in files["welded_rgb.ply"]
    assert files["nearest.i64"] == b"" and files["rgb.u8"] == b""


def test_hand_made_soup_clamps_rounds_and_welds_by_bits(program, tmp_path):
    tri, colour = fc.hand_soup()
    g = fs.grid(fc.HAND_DIMS, fc.HAND_ORIGIN, fc.HAND_VS, *fc.HAND_Z)
    # what the soup is for, stated with the spec: the clamp runs on both sides of every axis, halves round away from zero,
    # the zero-area face leaves a zero normal, and the vertices that differ in a zero's sign stay apart
    flat = tri.reshape(-1, 3)
    q = (flat - g["origin"]) / g["voxel_size"]
    i = fs.lround(q)
    i[:, 2] -= g["z_begin"]
    hi = np.array([g["dims"][0], g["dims"][1], g["z_end"] - g["z_begin"]])
    assert np.all((i < 0).any(axis=0)) and np.all((i >= hi).any(axis=0))
    halves = q[9:12].astype(np.float64)                # the fourth triangle
    assert np.all(np.abs(halves) % 1.0 == 0.5) and (halves > 0).any() and (halves < 0).any()
    assert np.array_equal(fs.lround(np.float32([2.5, -0.5, -1.5, 0.5])), [3, -1, -2, 1])
    verts, faces, normals = fs.weld(tri)
    assert faces[4, 0] == faces[4, 1] and np.array_equal(normals[faces[4, 0]], [0, 0, 0]) and np.array_equal(normals[faces[4, 2]], [0, 0, 0])
    assert np.count_nonzero(np.abs(normals).sum(axis=1) == 0) == 2
    assert np.array_equal(verts[faces[5, 0]], verts[faces[6, 0]]) and faces[5, 0] != faces[6, 0] and faces[5, 1] != faces[6, 1]
    assert faces[0, 1] == faces[1, 0] and faces[0, 2] == faces[1, 2] and len(verts) == 3 * len(tri) - 3
    files, _ = run(program, tmp_path, g, tri, colour)
    check(files, g, tri, colour)


def test_failure_codes(program, tmp_path):
    """A path that cannot be opened and a device that takes no byte: every writer says which."""
    tri, colour = fc.hand_soup()
    g = fs.grid(fc.HAND_DIMS, fc.HAND_ORIGIN, fc.HAND_VS, *fc.HAND_Z)
    missing = str(tmp_path / "no_such_directory" / "file")
    _, out = run(program, tmp_path, g, tri, colour, extra=(missing, "/dev/full"))
    lines = [line.split() for line in out.splitlines()]
    assert lines == [[missing] + [str(CANNOT_OPEN)] * 6, ["/dev/full"] + [str(SHORT_WRITE)] * 6]
