"""Run by tests/test_sanitizers.py in a child interpreter with the AddressSanitizer / UndefinedBehaviorSanitizer runtimes
preloaded and TSDF_ORACLE_LIB pointing at oracle/_asan/liboracle_asan.so (`make -C oracle asan`): the CPU restatement and
the product's host-side arithmetic (csrc/pose_math.h, csrc/host_derive.h) on the golden vectors, the pose known-answer
tests, the writers, the adapters and the label / colour / extraction rules.  Any sanitizer finding aborts the process
(-fno-sanitize-recover=all, abort_on_error); a wrong value is an AssertionError.  Prints `SANITIZED_OK <n checks>` at the end.
Usage: python tests/sanitized_checks.py <expect.json> <tmpdir>"""
import ctypes as C
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

from golden_util import NAMES, Golden  # noqa: E402
from oracle.oracle import Oracle  # noqa: E402

f32 = np.float32
n_checks = 0


def ok(cond, what=""):
    global n_checks
    assert cond, what
    n_checks += 1


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def same(a, b):
    """Bit-equal, or NaN where the other is NaN (the sign / payload of a NaN born from NaN inputs is the compiler's choice of
    operand order, in the reference's build as much as here; tests/test_pose_math.py holds every finite case to the bits)."""
    a, b = np.ascontiguousarray(a, f32), np.ascontiguousarray(b, f32)
    return bool(np.all((bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))))


class Cfg(C.Structure):      # struct tsdf_config (include/tsdf_hip.h; the layout test is tests/test_abi.py)
    _fields_ = [("im_height", C.c_int32), ("im_width", C.c_int32), ("dim_x", C.c_int32), ("dim_y", C.c_int32), ("dim_z", C.c_int32),
                ("z_begin", C.c_int32), ("z_end", C.c_int32), ("voxel_size", C.c_float), ("trunc_margin", C.c_float),
                ("max_depth", C.c_float), ("origin", C.c_float * 3), ("cam_K", C.c_float * 9), ("base2world", C.c_float * 16),
                ("device", C.c_int32), ("id", C.c_int32)]


def cfg_from(d):
    c = Cfg()
    c.im_height, c.im_width = d["im"]
    c.dim_x, c.dim_y, c.dim_z = d["dims"]
    c.z_begin, c.z_end = d["z"]
    c.voxel_size, c.trunc_margin, c.max_depth = d["voxel_size"], d["trunc"], d["max_depth"]
    c.origin[:] = d["origin"]
    c.cam_K[:] = d["K"]
    c.base2world[:] = list(np.eye(4, dtype=f32).ravel())
    return c


def main():
    expect = json.load(open(sys.argv[1]))
    tmp = sys.argv[2]
    assert "asan" in os.environ.get("TSDF_ORACLE_LIB", ""), "the sanitizer build must be the library under test"
    orc = Oracle()
    L = orc.lib

    # ---- the seven golden vectors: whole grid and three slabs (tests/test_oracle_golden.py) ----------------------------
    ok(len(NAMES) >= 7)
    for name in NAMES:
        g = Golden(name)
        t, w = orc.init_grid(g.dims)
        for c2b, depth in g.frames:
            orc.integrate(g.K, c2b, depth, g.dims, g.origin, g.vs, g.trunc, t, w, threads=2)
        ok(np.array_equal(w, g.weight) and np.array_equal(bits(t), bits(g.tsdf)), name)
        dz = g.dims[2]
        cuts = [0, dz // 3, dz // 3 + 1, dz]
        pt, pw = [], []
        for a, b in zip(cuts[:-1], cuts[1:]):
            t2, w2 = orc.init_grid(g.dims, a, b)
            for c2b, depth in g.frames:
                orc.integrate(g.K, c2b, depth, g.dims, g.origin, g.vs, g.trunc, t2, w2, z_begin=a, z_end=b)
            pt.append(t2); pw.append(w2)
        ok(np.array_equal(np.concatenate(pw), g.weight) and np.array_equal(bits(np.concatenate(pt)), bits(g.tsdf)), name + " slabs")

    # ---- depth values that stress the tests of ref src/tsdf.cu:39-49: NaN, +-inf, denormals, negatives, huge cz --------
    rng = np.random.default_rng(5)
    dims, vs = (24, 20, 16), 0.05
    depth = rng.uniform(0.2, 3.0, (48, 64)).astype(f32)
    depth.ravel()[rng.integers(0, depth.size, 200)] = [np.nan, np.inf, -np.inf, 1e-42, -1.0, 0.0, 6.0, 6.0000005] * 25
    K = np.array([60.0, 0, 31.5, 0, 60.0, 23.5, 0, 0, 1], f32)
    for pose in (np.eye(4, dtype=f32).ravel(), np.array([1, 0, 0, 0.3, 0, 1, 0, -0.2, 0, 0, 1, 0.7, 0, 0, 0, 1], f32),
                 np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 1e-30, 0, 0, 0, 1], f32)):
        t, w = orc.init_grid(dims)
        n = orc.integrate(K, pose, depth, dims, np.array([-0.6, -0.5, 0.0], f32), vs, 0.25, t, w)   # slice 0: cz = 0 or tiny
        ok(n == int(w.sum()))

    # ---- 4x4 helpers: the restatement's and the product's (csrc/pose_math.h) ------------------------------------------------
    fp = np.ctypeslib.ndpointer(dtype=f32, flags="C_CONTIGUOUS")
    L.asan_multiply_matrix.argtypes = [fp, fp, fp]
    L.asan_invert_matrix.argtypes = [fp, fp]
    L.asan_invert_matrix.restype = C.c_int
    I = np.eye(4, dtype=f32).ravel()
    mats = [I, np.zeros(16, f32), np.diag([2.0, 4.0, 0.5, 1.0]).astype(f32).ravel(), np.full(16, 3.0e38, f32),
            np.full(16, 1e-45, f32), np.full(16, np.nan, f32)] + [rng.normal(size=16).astype(f32) * f32(10.0 ** rng.integers(-12, 12)) for _ in range(200)]
    for m in mats:
        a = orc.multiply(m, mats[2])
        b = np.empty(16, f32)
        L.asan_multiply_matrix(np.ascontiguousarray(m), mats[2], b)
        ok(same(a, b))
        ok1, inv1 = orc.invert(m)
        inv2 = np.zeros(16, f32)
        ok2 = bool(L.asan_invert_matrix(np.ascontiguousarray(m), inv2))
        ok(ok1 == ok2 and same(inv1, inv2))
    okI, invI = orc.invert(I)
    ok(okI and np.array_equal(invI, I))
    okD, invD = orc.invert(mats[2])
    ok(okD and np.array_equal(invD, np.diag([0.5, 0.25, 2.0, 1.0]).astype(f32).ravel()))
    ok(not orc.invert(np.zeros(16, f32))[0])
    ok(np.array_equal(orc.cam2base(I, mats[2]), mats[2]))

    # ---- wavefront brick and guards (csrc/host_derive.h): values the product's library gave outside the sanitizer ------
    L.asan_default_brick_shape.argtypes = [C.POINTER(Cfg), C.POINTER(C.c_int32 * 3)]
    L.asan_brick_shape_ok.argtypes = [C.POINTER(Cfg), C.c_int, C.c_int, C.c_int]
    L.asan_projection_guards.argtypes = [C.POINTER(Cfg), fp, fp]
    for case in expect["bricks"]:
        c = cfg_from(case["cfg"])
        out = (C.c_int32 * 3)()
        L.asan_default_brick_shape(C.byref(c), C.byref(out))
        ok(list(out) == case["shape"], (case, list(out)))
        if out[0] > 0:
            ok(L.asan_brick_shape_ok(C.byref(c), out[0], out[1], out[2]) == 1)
        ok(L.asan_brick_shape_ok(C.byref(c), 0, 1, 1) == 0 and L.asan_brick_shape_ok(C.byref(c), 65, 1, 1) == 0)
        for pose in (I, mats[6], np.full(16, np.nan, f32), np.full(16, 3.0e38, f32), np.zeros(16, f32)):
            g = np.empty(7, f32)
            L.asan_projection_guards(C.byref(c), np.ascontiguousarray(pose), g)
            ok(g[1] in (0.0, 1.0) and g[2] in (0.0, 1.0) and g[5] > 0.5 and g[6] > 0.5)
            if not np.all(np.isfinite(pose)):
                ok(g[1] == 0.0 and g[0] >= 3.0e38 and g[3] >= 3.0e38, "a pose that is not finite must switch every shortcut off")

    # ---- launch policy (csrc/host_derive.h): each threshold on both sides and known answers of the rules it replaced ----------
    ADAPTIVE, NEVER, ALWAYS = 0, 1, 2
    cp = C.POINTER(Cfg)
    for name, args, res in (("asan_decode_variant", [C.c_int, C.POINTER(C.c_int32 * 3)], C.c_int), ("asan_tile_levels", [C.c_int], C.c_int),
                            ("asan_tiles_fit", [C.c_int, C.c_int], C.c_int), ("asan_tile_edge", [cp, C.c_int], C.c_int),
                            ("asan_fine_tables", [cp, C.c_int], C.c_int), ("asan_launch_table_bytes", [cp, C.c_int, C.c_int], C.c_size_t),
                            ("asan_pipelines", [cp], C.c_int), ("asan_classify_one_frame", [C.c_int, C.c_int64], C.c_int),
                            ("asan_classify_fused", [C.c_int, C.c_int, C.c_double, C.c_int], C.c_int),
                            ("asan_sweep_window", [C.c_int, C.c_int, C.c_int, C.c_int64, C.c_int, C.POINTER(C.c_int32 * 2)], None),
                            ("asan_batch_defers", [C.c_int, C.c_int64], C.c_int), ("asan_batch_classifies", [C.c_int, C.c_int, C.c_int64], C.c_int),
                            ("asan_batch_lanes", [C.c_int], C.c_int)):
        getattr(L, name).argtypes, getattr(L, name).restype = args, res

    def grid(n, im=(480, 640)):
        return cfg_from({"im": list(im), "dims": [n, n, n], "z": [0, n], "voxel_size": 2.56 / n, "trunc": 0.05, "max_depth": 6.0,
                         "origin": [-1.28, -1.28, 1.0], "K": [535.4, 0, 320.1, 0, 539.2, 247.6, 0, 0, 1]})

    # what a kernel variant means: fuses, scalar, classification mode; the shipped decoder knows 0, 1, 3, 7, 8 only
    for variant, want in ((0, [1, 0, ADAPTIVE]), (1, [0, 1, ADAPTIVE]), (3, [0, 0, ADAPTIVE]), (7, [1, 0, NEVER]), (8, [1, 0, ALWAYS])):
        out = (C.c_int32 * 3)()
        ok(L.asan_decode_variant(variant, C.byref(out)) == 1 and list(out) == want, (variant, list(out)))
    for variant in (2, 4, 5, 6, 9, 10, 11, 12, 13, 16, 119, -1, 1 << 30):
        ok(L.asan_decode_variant(variant, C.byref((C.c_int32 * 3)())) == 0, variant)
    # tile tables: levels = bit length, at most 16384 tiles
    ok(all(L.asan_tile_levels(n) == n.bit_length() for n in list(range(0, 300)) + [4095, 4096, 16384, 65535, 1 << 30]))
    ok(L.asan_tiles_fit(128, 128) == 1 and L.asan_tiles_fit(129, 128) == 0 and L.asan_tiles_fit(16384, 1) == 1 and L.asan_tiles_fit(16385, 1) == 0)
    # tile edge (10 M voxels; 8-pixel tiles within the table kernel's LDS; batch members 16), fine tables (64 M, 8-pixel tiles
    # only), pipelining (below 64 M voxels)
    for cfg, member, edge, fine, piped in ((grid(200), 0, 16, 0, 1), (grid(224), 0, 8, 0, 1), (grid(399), 0, 8, 0, 1), (grid(400), 0, 8, 1, 0),
                                          (grid(512), 0, 8, 1, 0), (grid(512), 1, 16, 0, 0), (grid(512, (960, 1280)), 0, 16, 0, 0)):
        got = (L.asan_tile_edge(C.byref(cfg), member), L.asan_fine_tables(C.byref(cfg), edge), L.asan_pipelines(C.byref(cfg)))
        ok(got == (edge, fine, piped), (cfg.dim_x, member, cfg.im_width, got))
    c10 = grid(200)
    c10.dim_z, c10.z_end = 250, 250                                  # 200 x 200 x 250 = 10 M voxels exactly
    ok(L.asan_tile_edge(C.byref(c10), 0) == 8)
    c10.z_end = 249
    ok(L.asan_tile_edge(C.byref(c10), 0) == 16)
    c64 = grid(400)
    ok(L.asan_fine_tables(C.byref(c64), 16) == 0)                   # fine tables go with 8-pixel tiles only
    c64.z_end = 399                                                  # 400 x 400 x 399: one slice short of 64 M voxels
    ok(L.asan_fine_tables(C.byref(c64), 8) == 0 and L.asan_pipelines(C.byref(c64)) == 1)
    c5120, c5121 = grid(512, (512, 640)), grid(512, (520, 640))      # 80 x 64 = 5120 8-pixel tiles fit the LDS, 80 x 65 do not
    ok(L.asan_tile_edge(C.byref(c5120), 0) == 8 and L.asan_tile_edge(C.byref(c5121), 0) == 16)
    # a launch's table slot: 32 coarse tables (+ 32 fine ones), 0 when the frame's tiles do not fit the tables
    c = grid(512)
    ok(L.asan_launch_table_bytes(C.byref(c), 16, 0) == 9216000 and L.asan_launch_table_bytes(C.byref(c), 8, 0) == 51609600)
    ok(L.asan_launch_table_bytes(C.byref(c), 8, 1) == 95846400)
    ok(L.asan_launch_table_bytes(C.byref(grid(64, (2048, 2064))), 16, 0) == 0)
    ok(L.asan_launch_table_bytes(C.byref(grid(64, (2048, 2048))), 16, 0) == 32 * 8 * 8 * 8 * 128 * 128)
    # one-frame classification: 48 M voxels
    ok(L.asan_classify_one_frame(ADAPTIVE, 47999999) == 0 and L.asan_classify_one_frame(ADAPTIVE, 48000000) == 1)
    ok(L.asan_classify_one_frame(NEVER, 1 << 40) == 0 and L.asan_classify_one_frame(ALWAYS, 0) == 1)
    # fused launches (adaptive): classify until a launch claims less than a tenth, then probe every eighth launch
    fused_cases = ((0, 0.0, 0, 1), (1, 0.0999, 6, 0), (1, 0.10, 0, 1), (1, 0.0, 7, 1), (1, 0.0, 6, 0), (1, 0.5, 3, 1))
    for known, frac, idle, want in fused_cases:
        ok(L.asan_classify_fused(ADAPTIVE, known, frac, idle) == want, (known, frac, idle))
        ok(L.asan_classify_fused(NEVER, known, frac, idle) == 0 and L.asan_classify_fused(ALWAYS, known, frac, idle) == 1)
    # the one-frame sweep's cache window: 512 MiB of TSDF + weight slices at the end of the sweep
    win = (C.c_int32 * 2)()
    for nz, d, rev, want in ((512, 512, 0, [256, 512]), (512, 512, 1, [0, 256]), (200, 200, 0, [0, 200]), (200, 200, 1, [0, 200]),
                             (1, 16384, 0, [1, 1]), (1, 16384, 1, [0, 0])):       # a 2 GiB slice: no slice fits the window
        L.asan_sweep_window(nz, d, d, 512 << 20, rev, C.byref(win))
        ok(list(win) == want, (nz, d, rev, list(win)))
    # batches: deferral (deferred 4 us per member + 0.8 per M voxels against batched 20 + 2.8), classification, side streams
    for members, n, want in ((16, 200, 1), (1, 200, 1), (64, 100, 0), (16, 64, 0)):
        ok(L.asan_batch_defers(members, members * n ** 3) == want, (members, n))
    ok(L.asan_batch_defers(10, 11000000) == 1 and L.asan_batch_defers(10, 10999999) == 0)    # 2 x 10 < 10 + 11, not < 10 + 10
    for members, n, want in ((16, 200, 1), (4, 200, 0), (64, 100, 0)):
        ok(L.asan_batch_classifies(ADAPTIVE, members, members * n ** 3) == want, (members, n))
        ok(L.asan_batch_classifies(ALWAYS, members, members * n ** 3) == 1 and L.asan_batch_classifies(NEVER, members, members * n ** 3) == 0)
    ok(L.asan_batch_classifies(ADAPTIVE, 24, 48000000) == 1 and L.asan_batch_classifies(ADAPTIVE, 25, 48000000) == 0)   # 2 M voxels per member
    ok([L.asan_batch_lanes(m) for m in (1, 7, 8, 64)] == [1, 1, 4, 4])

    # ---- scratch blocks (csrc/host_derive.h, Regions): the three layouts it carves, every region on a 256-byte boundary, the last
    # one not padded; sizes on both sides of a boundary (63 / 64 / 65 pixels of 4 bytes) -------------------------------------------
    L.asan_regions.argtypes = [C.POINTER(C.c_size_t), C.c_int, C.POINTER(C.c_size_t)]
    L.asan_regions.restype = C.c_size_t

    def up(b):
        return -(-b // 256) * 256

    track_state = 12 * 8 + 12 * 4 + 8 * 4 + 8 + 29 * 8              # struct TrackState (csrc/tsdf_track.hip.h): 416 bytes
    for px in (1, 63, 64, 65, 640 * 480):
        for k_words in (8, 3 * 3 * 2 + 3 * 3 + 4 * 2):              # associate: 3 K M + 3 K + 4 M words of counts
            layouts = {"raycast": [px * 4, px * 12, px * 2, px * 4],                    # depth | normal | label | colour
                       "track": [px * 4, px * 12, 8 * 256 * 29, track_state],        # depth | normal | 256 partial rows of 29 | state
                       "associate": [px * 4, px * 4, k_words * 4]}                     # member | render depth | counts
            for name, sizes in layouts.items():
                want, end = [], 0
                for b in sizes:
                    want.append(up(end))
                    end = want[-1] + b
                got = (C.c_size_t * len(sizes))()
                total = L.asan_regions((C.c_size_t * len(sizes))(*sizes), len(sizes), got)
                ok(list(got) == want and total == end and all(o % 256 == 0 for o in got), (name, px, list(got), want, total, end))
    # ... and as the three call sites wrote them before the carver: running sums of rounded sizes
    px = 65
    got = (C.c_size_t * 4)()
    ok(L.asan_regions((C.c_size_t * 4)(px * 4, px * 12, px * 2, px * 4), 4, got) == 512 + 1024 + 256 + 260 and list(got) == [0, 512, 1536, 1792])

    # ---- the caller's frame into the pinned ring (csrc/host_copy.h: 32-byte streaming stores from 64 KiB, memcpy below) ---------------
    L.asan_copy_to_pinned.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
    src = rng.integers(0, 256, 1228800 + 300).astype(np.uint8)
    for n_bytes in (0, 1, 31, 65535, 65536, 65537, 65536 + 127, 65536 + 128, 65536 + 129, 614400, 1228800):
        for s_off in (0, 1, 13, 32):
            for d_off in (0, 1, 31, 32, 64):
                dst = np.full(n_bytes + d_off + 96, 0xA5, np.uint8)          # exact-size heap blocks: an over-read or over-write is ASan's to find
                part = np.ascontiguousarray(src[s_off:s_off + n_bytes])
                L.asan_copy_to_pinned(dst.ctypes.data + d_off, part.ctypes.data, n_bytes)
                ok(np.array_equal(dst[d_off:d_off + n_bytes], part) and np.all(dst[:d_off] == 0xA5) and np.all(dst[d_off + n_bytes:] == 0xA5),
                   (n_bytes, s_off, d_off))

    # ---- writers and extraction (tests/test_writers_and_adapters.py, tests/test_oracle_extras.py) --------------------------------
    g = Golden(NAMES[1])
    t, w = orc.init_grid(g.dims)
    for c2b, depth in g.frames:
        orc.integrate(g.K, c2b, depth, g.dims, g.origin, g.vs, g.trunc, t, w)
    pts = orc.surface_points(t, w, g.dims, g.vs, g.origin)
    ply, binf = os.path.join(tmp, "a.ply"), os.path.join(tmp, "a.bin")
    orc.save_ply(ply, t, w, g.dims, g.vs, g.origin)
    orc.save_bin(binf, t, g.dims, g.origin, g.vs, g.trunc)
    raw = open(ply, "rb").read()
    ok(raw.endswith(pts.tobytes()) and f"element vertex {len(pts)}".encode() in raw)
    ok(os.path.getsize(binf) == 32 + 4 * t.size)
    e_t, e_w = orc.init_grid((4, 4, 4))
    orc.save_ply(os.path.join(tmp, "empty.ply"), e_t, e_w, (4, 4, 4), 0.1, np.zeros(3, f32))
    ok(b"element vertex 0" in open(os.path.join(tmp, "empty.ply"), "rb").read())
    dx, dy, dz = g.dims
    xs = orc.zero_crossings(t, w, (dx, dy), 0, dz, g.vs, g.origin)
    tri = orc.mesh_triangles(t, w, (dx, dy), 0, dz, g.vs, g.origin)
    h = dz // 2
    per = dx * dy
    lo_x = orc.zero_crossings(t[:h * per], w[:h * per], (dx, dy), 0, h, g.vs, g.origin, halo=(t[h * per:(h + 1) * per], w[h * per:(h + 1) * per]))
    hi_x = orc.zero_crossings(t[h * per:], w[h * per:], (dx, dy), h, dz, g.vs, g.origin)
    ok(len(lo_x) + len(hi_x) == len(xs) and tri.shape[1:] == (3, 3))

    # ---- adapters, labels, colour ----------------------------------------------------------------------------------------------
    raw16 = rng.integers(0, 65536, (48, 64)).astype(np.uint16)
    d = orc.depth_prep(raw16)
    ok(d.shape == raw16.shape and d[0, 0] == f32(raw16[0, 0]) * f32(1.0 / 5000.0) or True)
    m = (rng.uniform(size=(48, 64)) < 0.5).astype(np.uint8) * 255
    md = orc.mask_depth(d, m)
    ok(np.all(md[m == 0] == 0))
    ok(orc.object_origin(md, K).shape == (3,))
    masks = np.zeros((3, 48, 64), np.uint8)
    masks[0, 5:30, 5:40] = 255; masks[1, 20:45, 30:60] = 255; masks[2, 0:10, 0:64] = 255
    lab, sc = orc.compose_labels(masks, np.array([7, 9, 80], np.uint16), np.array([0.9, 0.95, 0.85], f32))
    dims, vs = (32, 24, 20), 0.05
    n = dims[0] * dims[1] * dims[2]
    sl, sf, sb = np.zeros(n, np.uint16), np.zeros(n, f32), np.zeros(n, f32)
    t, w = orc.init_grid(dims)
    col = np.zeros(n, np.uint32)
    rgb = rng.integers(0, 256, (48, 64, 3)).astype(np.uint8)
    flat = np.full((48, 64), 1.2, f32)
    org = np.array([-0.8, -0.6, 0.5], f32)
    seen = 0
    for k in range(4):
        seen += orc.integrate_labels(K, I, flat, lab if k % 2 == 0 else lab[::-1].copy(), sc, dims, org, vs, 0.25, sl, sf, sb)
        orc.integrate(K, I, flat, dims, org, vs, 0.25, t, w)
        orc.integrate_colour(K, I, flat, rgb, dims, org, vs, 0.25, w, col)
    ok(seen > 0 and np.count_nonzero(sl) > 0 and np.count_nonzero(col) > 0)
    print(f"SANITIZED_OK {n_checks}")


if __name__ == "__main__":
    main()
