// launch_geometry_check.cpp -- a slab's launch geometry (semantic_slam_amd/csrc/launch_geometry.h, and the table slot's layout
// in host_derive.h) without a device: a stand-alone program (tests/test_launch_geometry.py builds and runs it).  Every expectation
// below is stated from the rule, not computed with the function under test:
//   a grid of g workgroups of k items covers n items when g * k >= n and its last workgroup is not empty, (g - 1) * k < n; a
//   slab without slices launches nothing; a quad is 4 voxels, a chunk 256 voxels of a slice, a summary word belongs to a chunk
//   of a slab whose rows divide into quads; rows of a multiple of 256 voxels are mapped row by row (nseg segments), all others
//   flat; a brick is q quads x r rows x s slices, a workgroup takes four of them, the class table has a byte per wavefront of
//   the brick grid; (x * magic) >> 16 divides a lane index; a table slot holds 32 coarse tables, then 32 fine ones; a sub-list
//   of the work list holds every brick of every super-brick dealt to it.
// Prints one line per failed expectation and exits with their number (0 = all good), then "checked N cases".
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "launch_geometry.h"

using namespace tsdf_host;

static int failures = 0;
static const char *g_what = "";
static long long g_ctx[6];

static void expect(bool ok, const char *what)
{
    if (ok) return;
    if (++failures > 50) return;
    std::printf("FAILED %s (%s): %lld %lld %lld | %lld %lld %lld\n", what, g_what, g_ctx[0], g_ctx[1], g_ctx[2], g_ctx[3], g_ctx[4], g_ctx[5]);
}

// g groups of k cover n items, the last group not empty; nothing for nothing
static bool covers(int64_t g, int64_t k, int64_t n) { return g * k >= n && (n == 0 ? g == 0 : (g - 1) * k < n); }

static tsdf_config config(int dx, int dy, int z0, int depth, int W = 83, int H = 60)
{
    tsdf_config c;
    std::memset(&c, 0, sizeof c);
    c.im_width = W; c.im_height = H;
    c.dim_x = dx; c.dim_y = dy; c.dim_z = z0 + depth + 2; c.z_begin = z0; c.z_end = z0 + depth;
    c.voxel_size = 0.004f; c.trunc_margin = 0.02f; c.max_depth = 6.0f;
    c.cam_K[0] = 535.4f; c.cam_K[2] = 320.1f; c.cam_K[4] = 539.2f; c.cam_K[5] = 247.6f; c.cam_K[8] = 1.0f;
    return c;
}

// levels of a sparse table over n tiles: 1, 2, 4, ... tiles per entry while the entry fits
static int levels_by_rule(int n) { int l = 0; while ((1 << l) <= n) ++l; return l; }

// ---- the views and grids of one slab that do not depend on the brick ----
static void check_slab(const tsdf_config &c, const SlabGeometry &g)
{
    const int64_t nz = c.z_end - c.z_begin, slice = (int64_t)c.dim_x * c.dim_y;
    const bool quads = c.dim_x % 4 == 0;
    expect(g.nz == nz && g.dim_x == c.dim_x && g.dim_y == c.dim_y && g.n_vox == slice * nz, "slab dims");
    expect(g.quad_rows == quads, "rows divide into quads");
    expect(g.flat == (c.dim_x % 256 != 0), "flat unless rows are a multiple of 256 voxels");
    expect(((int64_t)g.nseg * 256 == c.dim_x) == !g.flat, "nseg * 256 == dim_x exactly when not flat");
    expect(covers(g.chunks_per_slice, 256, slice), "chunks of 256 voxels cover a slice");
    expect(g.n_flags == (quads ? (uint64_t)g.chunks_per_slice * (uint64_t)nz : 0u), "a summary word per chunk and slice, quad rows only");
    if (quads) expect((int64_t)g.quads_per_row * 4 == c.dim_x && (int64_t)g.quads_per_slice * 4 == slice, "quads");
    // scalar rows: 64 voxels of a row per wavefront, 4 rows per workgroup
    const Grid3 sc = grid_scalar_rows(g);
    expect(covers(sc.x, 64, c.dim_x) && covers(sc.y, 4, c.dim_y) && sc.z == (unsigned)nz, "scalar rows");
    // quad rows: 64 quads of a row per wavefront, 4 or 8 rows per workgroup
    const int64_t row_quads = (c.dim_x + 3) / 4;
    for (const int rows : {4, 8}) {
        const Grid3 q = grid_quad_rows(g, rows);
        expect(covers(q.x, 64, row_quads) && covers(q.y, rows, c.dim_y) && q.z == (unsigned)nz, "quad rows");
        expect(q.y <= 65535u && q.z <= 65535u, "quad rows fit a launch");
        expect(q.empty() == (nz == 0), "no slices, no launch (quad rows)");
    }
    // flat: a chunk per wavefront, four per workgroup; the pass that recomputes the summary runs the same grid
    for (const Grid3 &f : {grid_flat(g), grid_recompute_flags(g)}) {
        expect(covers(f.x, 4, g.chunks_per_slice) && f.y == 1u && f.z == (unsigned)nz, "flat");
        expect(f.empty() == (nz == 0), "no slices, no launch (flat)");
    }
    expect(sc.empty() == (nz == 0), "no slices, no launch (scalar)");
    // grid-stride passes: a workgroup per 256 words / quads while there are fewer than 2048 of them, then 2048
    const Grid3 fw = grid_summary_words(g), fl = grid_fill(g);
    const uint64_t word_groups = (g.n_flags + 255) / 256, quad_groups = ((uint64_t)g.n_vox / 4 + 255) / 256;
    expect(fw.x == (word_groups < 2048 ? word_groups : 2048) && fw.y == 1u && fw.z == 1u, "forget_runs");
    expect(fw.empty() == (g.n_flags == 0), "no words, no pass");
    expect(fl.x == (quad_groups < 1 ? 1 : quad_groups < 2048 ? quad_groups : 2048) && fl.y == 1u && fl.z == 1u, "fill_grid");
    expect(g.xgroups(1) == c.dim_x && g.xgroups(4) == row_quads, "lanes along a row");
}

// ---- the brick view, the brick grid, the lane map and the work list of one slab under one brick ----
static void check_brick(const tsdf_config &c, int q, int r, int s)
{
    const SlabGeometry g = slab_geometry(c, 16, false, q, r, s);
    const int64_t nz = c.z_end - c.z_begin;
    g_ctx[3] = q; g_ctx[4] = r; g_ctx[5] = s;
    expect(g.brick_s >= 1, "a brick has a slice at least");
    expect(covers(g.nz_groups, g.brick_s, nz), "slice groups cover the slices");
    if (q == 0) {
        const WorkListLayout none = work_list_layout(c, g, 0);
        expect(g.bricks_per_group == 0 && g.brick_groups == 0 && none.n_super == 0 && none.total == 0 && none.fits, "no brick view, no list");
        return;
    }
    expect(g.brick_q == q && g.brick_r == r && g.brick_s == s, "the brick as given");
    expect((int64_t)g.bricks_per_group * q * 4 == c.dim_x, "bricks along a row");
    expect(covers(g.brick_groups, r, c.dim_y), "row groups cover the rows");
    const BrickGrid bg = brick_grid(g);
    expect(covers(bg.grid.x, 4, (int64_t)g.bricks_per_group * g.brick_groups) && bg.grid.y == 1u && bg.grid.z == (unsigned)g.nz_groups, "brick grid");
    expect(bg.class_elems == (uint64_t)4 * bg.grid.x * bg.grid.z, "a class per wavefront of the brick grid");
    expect((int)bg.grid.x == brick_blocks(g), "blocks");
    expect(bg.grid.empty() == (nz == 0), "no slices, no launch (bricks)");
    // the lane map, restated from tsdf_multiframe.hip.h, "lane -> (slice, row, quad)"
    {
        const int per = q * r;
        uint64_t seen = 0;      // a bit per (slice, row, quad) of the brick: 64 at most
        for (unsigned lane = 0; lane < 64; ++lane) {
            const int zz = (int)((lane * (unsigned)g.brick_per_magic) >> 16), rem = (int)lane - zz * per;
            const int rr = (int)(((unsigned)rem * (unsigned)g.brick_q_magic) >> 16), qq = rem - rr * q;
            if ((int)lane < q * r * s) {
                expect(qq >= 0 && qq < q && rr >= 0 && rr < r && zz >= 0 && zz < s, "a lane of the brick lands inside it");
                const uint64_t bit = (uint64_t)1 << (((zz * r + rr) * q + qq) & 63);
                expect(!(seen & bit), "two lanes on one quad");
                seen |= bit;
            } else {
                expect(zz >= s, "a lane beyond the brick lands on a slice beyond it");
            }
        }
    }
    // the work list: super-bricks of 4 x 2 x 1 bricks; dealt to 64 sub-lists; a sub-list holds the bricks of all it can get
    const double vs = c.voxel_size;
    struct Wedge { int mode; float oy, oz, fy; int want_o, want_fy; };
    const Wedge wedges[] = {
        {0, 0.0f, 0.0f, 539.2f, 0, 539},
        {1, (float)(-4.0e4 * vs), (float)(-4.0e4 * vs), 0.2f, -30000, 1},   {1, (float)(4.0e4 * vs), (float)(4.0e4 * vs), 1.0e6f, 30000, 16000},
        {2, (float)(-4.0e4 * vs), (float)(-4.0e4 * vs), 1.0e6f, -30000, 16000}, {2, (float)(4.0e4 * vs), (float)(4.0e4 * vs), 0.2f, 30000, 1},
        {3, (float)(-4.0e4 * vs), (float)(-4.0e4 * vs), 0.2f, -30000, 1},   {3, (float)(4.0e4 * vs), (float)(4.0e4 * vs), 1.0e6f, 30000, 16000},
        {3, (float)(-4.0e4 * vs), (float)(4.0e4 * vs), 1.0e6f, -30000, 16000},
    };
    for (const Wedge &wd : wedges) {
        if (wd.mode != 0 && c.z_begin == 0) continue;      // the wedge modes where the slab's first slice enters the key
        tsdf_config cw = c;
        cw.origin[1] = wd.oy; cw.origin[2] = wd.oz; cw.cam_K[4] = wd.fy;
        const WorkListLayout w = work_list_layout(cw, g, wd.mode);
        expect(w.wedge_mode == wd.mode && w.wedge_oy == wd.want_o && w.fy_px == wd.want_fy, "wedge key: clamped and rounded");
        if (wd.mode != 0) expect(w.wedge_oz == (wd.oz < 0 ? -30000 : 30000), "wedge key: z clamp");
        expect(w.super_h == 2 * r && w.super_d == s, "a super-brick's height and depth in voxels");
        expect(covers(w.nsx, 4, g.bricks_per_group) && covers(w.nsy, 2, g.brick_groups) && covers(w.nsz, 1, g.nz_groups), "super-bricks cover the bricks");
        expect(w.n_super == (int64_t)w.nsx * w.nsy * w.nsz, "n_super");
        int64_t per[64] = {};
        int64_t sum = 0, most = 0;
        bool in_range = true;
        for (int64_t id = 0; id < w.n_super; ++id) {      // the index order of classify_brick_list: slice groups fastest, then x, then y
            const int sz = (int)(id % w.nsz), t = (int)(id / w.nsz), sx = t % w.nsx, sy = t / w.nsx;
            const unsigned b = list_bucket((unsigned)id, sx, sy, sz, w.wedge_mode, w.wedge_oy, w.wedge_oz, w.super_h, w.super_d, w.fy_px);
            if (b >= 64u) { in_range = false; break; }
            ++per[b];
        }
        for (const int64_t n : per) { sum += n; most = n > most ? n : most; }
        expect(in_range, "a bucket below kListBuckets");
        expect(sum == w.n_super, "every super-brick in one sub-list");
        expect(w.bucket_supers == most && w.bucket_cap == most * 8 && w.total == w.bucket_cap * 64 && w.fits, "capacity: the fullest sub-list's bricks");
        const Grid3 gc = grid_classify_list(w), gl = grid_brick_list(w);
        expect(covers(gc.x, 4, w.n_super) && gc.y == 1u && gc.z == 1u, "a wavefront per super-brick");
        expect(gl.x == (uint64_t)((w.bucket_cap + 3) / 4 + 1) * 64 && gl.y == 1u && gl.z == 1u, "front and back groups of every sub-list");
    }
}

int main()
{
    long cases = 0;
    expect(kListBuckets == 64 && kSuperBX == 4 && kSuperBY == 2 && kSuperBZ == 1 && kSuperBricks == 8, "constants of the work list");

    // ---- the sweep: shapes x slab depths x z_begin x (every brick brick_shape_ok accepts + the library's choice) ----
    const int dims_x[] = {1, 3, 4, 8, 36, 37, 100, 252, 256, 260, 512, 1024};
    const int dims_y[] = {1, 2, 3, 4, 5, 7, 8, 9, 13, 48, 200};
    const int depths[] = {0, 1, 2, 3, 8, 9};
    for (const int dx : dims_x) for (const int dy : dims_y) for (const int depth : depths) for (const int z0 : {0, 5}) {
        const tsdf_config c = config(dx, dy, z0, depth);
        g_what = "sweep"; g_ctx[0] = dx; g_ctx[1] = dy; g_ctx[2] = depth * 100 + z0; g_ctx[3] = g_ctx[4] = g_ctx[5] = 0;
        expect(config_limits_ok(c) == ConfigLimit::Ok, "an ordinary shape is admitted");
        check_slab(c, slab_geometry(c, 16, false, 0, 0, 1));
        ++cases;
        for (int q = 1; q <= 64; ++q) for (int r = 1; q * r <= 64; ++r) for (int s = 1; q * r * s <= 64; ++s) {
            if (!brick_shape_ok(c, q, r, s)) continue;
            check_brick(c, q, r, s);
            ++cases;
        }
        int q = -1, r = -1, s = -1;
        choose_brick_default(c, q, r, s);
        expect(q == 0 ? dx % 4 != 0 : brick_shape_ok(c, q, r, s), "the library's choice is legal, or none for rows that are no quads");
        check_brick(c, q, r, s);
        ++cases;
    }

    // ---- magic division: every divisor a legal brick gives (q and q * r, up to 64), every lane index ----
    g_what = "magic";
    for (int d = 1; d <= 64; ++d) {
        // a brick of d quads x 1 row: both magic numbers divide by d
        const tsdf_config c = config(4 * d, 8, 0, 4);
        const SlabGeometry g = slab_geometry(c, 16, false, d, 1, 1);
        g_ctx[0] = d;
        expect(brick_shape_ok(c, d, 1, 1), "d quads x 1 x 1 is a legal brick");
        for (unsigned x = 0; x < 64; ++x)
            expect((int)((x * (unsigned)g.brick_q_magic) >> 16) == (int)x / d && (int)((x * (unsigned)g.brick_per_magic) >> 16) == (int)x / d, "(x * magic) >> 16 == x / d");
        ++cases;
    }

    // ---- the corners of what config_limits_ok admits, and each limit plus one ----
    g_what = "limits";
    {
        struct Corner { int dx, dy, depth; };
        const int64_t slice_max = ((int64_t)1 << 31) - 1024;
        const Corner ok[] = {{8, 262140, 3}, {260, 9, 65535}, {8188, 262140, 65535}, {(int)(slice_max / 16384), 16384, 2}, {(int)slice_max, 1, 1}};
        for (const Corner &k : ok) {
            tsdf_config c = config(k.dx, k.dy, 0, k.depth);
            g_ctx[0] = k.dx; g_ctx[1] = k.dy; g_ctx[2] = k.depth;
            expect(config_limits_ok(c) == ConfigLimit::Ok, "a corner is admitted");
            int q, r, s;
            choose_brick_default(c, q, r, s);
            const SlabGeometry g = slab_geometry(c, 16, false, q, r, s);
            check_slab(c, g);
            expect((int64_t)g.quads_per_slice * 4 <= slice_max && (int64_t)g.chunks_per_slice * 256 < ((int64_t)1 << 31), "a slice's quads and chunks are 32-bit");
            if (q > 0) {
                const BrickGrid bg = brick_grid(g);
                expect(covers(bg.grid.x, 4, (int64_t)g.bricks_per_group * g.brick_groups) && bg.grid.z <= 65535u, "brick grid at a corner");
                expect(bg.class_elems == (uint64_t)4 * bg.grid.x * bg.grid.z, "class table at a corner");
            }
            ++cases;
        }
        // the largest slab of all has more bricks than the work list's index holds: refused, and without being counted
        {
            tsdf_config c = config(8188, 262140, 0, 65535);
            const SlabGeometry g = slab_geometry(c, 16, false, 2, 4, 8);
            const WorkListLayout w = work_list_layout(c, g, 0);
            expect(!w.fits && w.total > 0x7fffffffll - 1024, "a list past the 32-bit index is refused");
            ++cases;
        }
        struct Refused { int dx, dy, dz, z0, z1, W, H; float vs, trunc; ConfigLimit want; };
        const Refused bad[] = {
            {0, 8, 8, 0, 8, 83, 60, 0.004f, 0.02f, ConfigLimit::GridDims},
            {8, 8, 8, 2, 9, 83, 60, 0.004f, 0.02f, ConfigLimit::SlabRange},
            {8, 8, 8, 3, 2, 83, 60, 0.004f, 0.02f, ConfigLimit::SlabRange},
            {8, 8, 8, 0, 8, 32768, 32769, 0.004f, 0.02f, ConfigLimit::ImageSize},      // 2^30 pixels + 32768
            {8, 8, 8, 0, 8, 83, 0, 0.004f, 0.02f, ConfigLimit::ImageSize},
            {8, 8, 8, 0, 8, 83, 60, 0.0f, 0.02f, ConfigLimit::VoxelAndTrunc},
            {8, 262141, 8, 0, 8, 83, 60, 0.004f, 0.02f, ConfigLimit::LaunchLimits},
            {8, 8, 65536, 0, 65536, 83, 60, 0.004f, 0.02f, ConfigLimit::LaunchLimits},
            {(int)slice_max + 1, 1, 8, 0, 8, 83, 60, 0.004f, 0.02f, ConfigLimit::SliceVoxels},
            {(int)(slice_max / 16384), 16385, 8, 0, 8, 83, 60, 0.004f, 0.02f, ConfigLimit::SliceVoxels},
            // the order: the first limit that fails is the one reported
            {0, 262141, 8, 0, 9, 0, 0, 0.0f, 0.0f, ConfigLimit::GridDims},
            {8, 262141, 8, 0, 9, 0, 0, 0.0f, 0.0f, ConfigLimit::SlabRange},
            {8, 262141, 8, 0, 8, 0, 0, 0.0f, 0.0f, ConfigLimit::ImageSize},
            {8, 262141, 8, 0, 8, 83, 60, 0.0f, 0.0f, ConfigLimit::VoxelAndTrunc},
            {(int)slice_max, 262141, 8, 0, 8, 83, 60, 0.004f, 0.02f, ConfigLimit::LaunchLimits},
        };
        for (const Refused &k : bad) {
            tsdf_config c = config(k.dx, k.dy, 0, 1, k.W, k.H);
            c.dim_z = k.dz; c.z_begin = k.z0; c.z_end = k.z1; c.voxel_size = k.vs; c.trunc_margin = k.trunc;
            g_ctx[0] = k.dx; g_ctx[1] = k.dy; g_ctx[2] = (long long)k.want;
            expect(config_limits_ok(c) == k.want, "a limit plus one is refused, with the limit's name");
            ++cases;
        }
        {   // the image limit itself is admitted
            tsdf_config c = config(8, 8, 0, 8, 32768, 32768);
            expect(config_limits_ok(c) == ConfigLimit::Ok, "2^30 pixels are admitted");
            ++cases;
        }
    }

    // ---- image sizes: the tile view, the strip grids, the table slot ----
    g_what = "image";
    {
        struct Image { int W, H; bool fits16, fits8; };
        const Image images[] = {{83, 60, true, true}, {640, 480, true, true}, {641, 479, true, true}, {2048, 2064, false, false}, {1030, 1030, true, false}};
        for (const Image &im : images) for (const int tile : {16, 8}) for (const bool fine : {false, true}) {
            if (fine && tile != 8) continue;
            const tsdf_config c = config(8, 8, 0, 8, im.W, im.H);
            const SlabGeometry g = slab_geometry(c, tile, fine, 0, 0, 1);
            g_ctx[0] = im.W; g_ctx[1] = im.H; g_ctx[2] = tile; g_ctx[3] = fine;
            expect(g.tile == tile && covers(g.tiles_w, tile, im.W) && covers(g.tiles_h, tile, im.H), "tiles cover the image");
            expect(g.tile_inv * (float)tile == 1.0f, "tile_inv");
            expect(g.fine == fine && (fine ? covers(g.fine_w, 4, im.W) && covers(g.fine_h, 4, im.H) : g.fine_w == 0 && g.fine_h == 0), "fine tiles cover the image");
            for (const int frames : {1, 32}) {
                const Grid3 st = grid_tile_strips(g.tiles_w, g.tiles_h, tile, frames);
                // a strip is 64 pixels of a tile row; a wavefront per strip, four per workgroup
                int strips_per_row = 0;
                while (strips_per_row * 64 < g.tiles_w * tile) ++strips_per_row;
                expect(covers(st.x, 4, (int64_t)strips_per_row * g.tiles_h) && st.y == (unsigned)frames && st.z == 1u, "strips cover the tile rows");
            }
            const bool fits = tile == 16 ? im.fits16 : im.fits8;
            expect(fits == ((int64_t)g.tiles_w * g.tiles_h <= 16384), "the case is what it says");
            const TableSlotLayout l = table_slot_layout(c, tile, fine);
            if (!fits) {
                expect(l.bytes == 0 && launch_table_bytes(c, tile, fine) == 0, "tiles that do not fit: no slot");
            } else {
                // regions, in order: 32 coarse tables from 0, then 32 fine ones; disjoint; bytes = the end of the last one
                const uint64_t coarse = (uint64_t)levels_by_rule(g.tiles_w) * levels_by_rule(g.tiles_h) * g.tiles_w * g.tiles_h;
                const uint64_t fine_e = fine ? (uint64_t)9 * g.fine_w * g.fine_h : 0;
                expect(l.coarse_elems == coarse && l.fine_elems == fine_e, "elements per table");
                uint64_t end = 0;
                bool ordered = true;
                for (int f = 0; f < 32; ++f) { ordered = ordered && (uint64_t)f * l.coarse_elems >= end; end = (uint64_t)(f + 1) * l.coarse_elems; }
                ordered = ordered && l.fine_begin >= end;
                end = l.fine_begin;
                for (int f = 0; f < 32; ++f) { ordered = ordered && l.fine_begin + (uint64_t)f * l.fine_elems >= end; end = l.fine_begin + (uint64_t)(f + 1) * l.fine_elems; }
                expect(ordered, "regions in order and disjoint");
                expect(l.fine_begin == 32 * coarse, "no gap in front of the fine tables");
                expect(l.bytes == end * 8 && launch_table_bytes(c, tile, fine) == l.bytes, "bytes = the end of the last region");
            }
            ++cases;
        }
        // what the function gave before the layout existed (640 x 480)
        const tsdf_config c = config(8, 8, 0, 8, 640, 480);
        expect(launch_table_bytes(c, 16, false) == 9216000u, "640 x 480, tile 16");
        expect(launch_table_bytes(c, 8, false) == 51609600u, "640 x 480, tile 8");
        expect(launch_table_bytes(c, 8, true) == 95846400u, "640 x 480, tile 8 with fine tables");
        cases += 3;
    }

    // ---- the work list's 32-bit guard: trips exactly where the total passes 2^31 - 1 - 1024 ----
    g_what = "guard";
    {
        WorkListLayout w;
        work_list_capacity(w, 4194301);      // x 8 bricks x 64 sub-lists = 2147482112 <= 2147482623
        expect(w.total == 2147482112ll && w.fits, "the last total that fits");
        ++cases;
        work_list_capacity(w, 4194302);      // 2147482624: one past
        expect(w.total == 2147482624ll && !w.fits, "the first total that does not");
        ++cases;
        expect(kMaxWorkListEntries == 2147482623ll, "2^31 - 1 - 1024");
    }

    if (failures > 50) std::printf("... and %d more\n", failures - 50);
    std::printf("checked %ld cases\n", cases);
    return failures > 255 ? 255 : failures;
}
