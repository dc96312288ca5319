// launch_geometry.h -- what every launch of the fusion path takes from the slab: its geometry, derived once per handle.
// Plain C++ (no HIP, no device types), on top of host_derive.h: the limits a configuration must keep (config_limits_ok), the
// record of a slab's views (SlabGeometry: rows, quads and chunks, the summary words, the wavefront brick with the lane map's
// magic numbers, the depth tiles), the grid of every mapping the product launches with the buffer sizes that go with it, and the
// layout of the brick work list with list_bucket, the one function here that the kernels run too.  tsdf_capi.hip builds the
// record at creation and wherever the brick shape changes; the launch sites read it and compute nothing of this themselves.
// tests/launch_geometry_check.cpp sweeps all of it on the CPU under -fsanitize=address,undefined: a grid that overhangs an
// allocation is a memory fault on the device, and here it is a failed comparison.
// Last, the two launch decisions that go with the geometry: what a launch keeps of the summary words with the host's record of
// them (SummaryRecord), and the kernel one frame runs (one_frame); tests/summary_duty_check.cpp walks both the same way.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>

#include "host_derive.h"

namespace tsdf_host {

// ---- limits --------------------------------------------------------------------------------------------------------
// What tsdf_create refuses, in the order it looks: with these kept, every grid below fits a launch (65535 in y and z), a
// slice's voxels and a quad's index fit 32 bits and the image's pixels fit a table index.
enum class ConfigLimit { Ok, GridDims, SlabRange, ImageSize, VoxelAndTrunc, LaunchLimits, SliceVoxels };

constexpr int kMaxDimY = 65535 * 4, kMaxSlices = 65535;
constexpr int64_t kMaxSliceVoxels = ((int64_t)1 << 31) - 1024, kMaxImagePixels = (int64_t)1 << 30;

inline ConfigLimit config_limits_ok(const tsdf_config &c)
{
    if (c.dim_x <= 0 || c.dim_y <= 0 || c.dim_z <= 0) return ConfigLimit::GridDims;
    if (c.z_begin < 0 || c.z_end < c.z_begin || c.z_end > c.dim_z) return ConfigLimit::SlabRange;
    if (c.im_height <= 0 || c.im_width <= 0 || (int64_t)c.im_height * c.im_width > kMaxImagePixels) return ConfigLimit::ImageSize;
    if (!(c.voxel_size > 0.0f) || !(c.trunc_margin > 0.0f)) return ConfigLimit::VoxelAndTrunc;
    if (c.dim_y > kMaxDimY || (c.z_end - c.z_begin) > kMaxSlices) return ConfigLimit::LaunchLimits;
    if ((int64_t)c.dim_x * c.dim_y > kMaxSliceVoxels) return ConfigLimit::SliceVoxels;
    return ConfigLimit::Ok;
}

// ---- the slab's views ----------------------------------------------------------------------------------------------
inline int ceil_div(int a, int b) { return (a + b - 1) / b; }

struct SlabGeometry {
    int dim_x = 0, dim_y = 0, nz = 0;   // the slab: nz slices of dim_y rows of dim_x voxels
    int64_t n_vox = 0;
    // rows: quad_rows = a row divides into quads (4 voxels, 16 bytes), what every kernel but the scalar one needs; flat = its
    // rows are no multiple of 256 voxels, so summary-keeping launches map a slice's quads linearly (256-voxel chunks) instead of
    // row by row; nseg = 256-voxel segments per row when they are (else 0)
    bool quad_rows = false, flat = false;
    int nseg = 0;
    int chunks_per_slice = 0;           // ceil(dim_x * dim_y / 256)
    int quads_per_row = 0, quads_per_slice = 0;   // rounded down (exact for quad rows)
    size_t n_flags = 0;                 // summary words: one per chunk and slice for quad rows, none otherwise
    // brick view (tsdf_multiframe.hip.h, BRICK): brick_q quads x brick_r rows x brick_s slices per wavefront, q = 0: none
    // (s >= 1 always); bricks_per_group along a row, brick_groups of rows per slice, nz_groups of slices; the magic numbers
    // divide a lane index below 64 by q * r and by q: (x * magic) >> 16 == x / d for 65536 / d + 1
    int brick_q = 0, brick_r = 0, brick_s = 1;
    int bricks_per_group = 0, brick_groups = 0, nz_groups = 0;
    int brick_q_magic = 0, brick_per_magic = 0;
    // tile view: depth tiles of `tile` pixels (tile_edge) and, beside them, fine ones of kFineTile pixels (fine_tables)
    int tile = 0, tiles_w = 0, tiles_h = 0;
    float tile_inv = 0.0f;
    bool fine = false;
    int fine_w = 0, fine_h = 0;

    int xgroups(int vx) const { return ceil_div(dim_x, vx); }   // lanes along a row at vx voxels per lane
};

// tile: 8 or 16.  (brick_q, brick_r, brick_s): a shape brick_shape_ok accepts, or brick_q = 0 for none.
inline SlabGeometry slab_geometry(const tsdf_config &c, int tile, bool fine, int brick_q, int brick_r, int brick_s)
{
    SlabGeometry g;
    g.dim_x = c.dim_x; g.dim_y = c.dim_y; g.nz = c.z_end - c.z_begin;
    g.n_vox = slab_voxels(c);
    g.quad_rows = c.dim_x % 4 == 0;
    g.flat = c.dim_x % 256 != 0;
    g.nseg = g.flat ? 0 : c.dim_x / 256;
    g.chunks_per_slice = (int)(((int64_t)c.dim_x * c.dim_y + 255) / 256);
    g.quads_per_row = c.dim_x / 4;
    g.quads_per_slice = (int)((int64_t)c.dim_x * c.dim_y / 4);
    g.n_flags = g.quad_rows ? (size_t)g.chunks_per_slice * (size_t)g.nz : 0;
    g.brick_q = brick_q; g.brick_r = brick_r; g.brick_s = brick_s > 0 ? brick_s : 1;
    g.nz_groups = ceil_div(g.nz, g.brick_s);
    if (brick_q > 0) {
        g.bricks_per_group = g.quads_per_row / brick_q;
        g.brick_groups = ceil_div(c.dim_y, brick_r);
        g.brick_q_magic = 65536 / brick_q + 1;
        g.brick_per_magic = 65536 / (brick_q * brick_r) + 1;
    }
    g.tile = tile;
    g.tiles_w = tiles_along(c.im_width, tile); g.tiles_h = tiles_along(c.im_height, tile);
    g.tile_inv = 1.0f / (float)tile;
    g.fine = fine;
    g.fine_w = fine ? tiles_along(c.im_width, kFineTile) : 0;
    g.fine_h = fine ? tiles_along(c.im_height, kFineTile) : 0;
    return g;
}

// ---- grids ---------------------------------------------------------------------------------------------------------
// Workgroups of a launch.  Every kernel of the fusion path runs workgroups of 64 x 4 lanes (four wavefronts), the summary passes
// below 256 x 1.  A slab without slices gives an empty grid: nothing is launched.
struct Grid3 {
    unsigned x = 0, y = 1, z = 1;
    bool empty() const { return x == 0 || y == 0 || z == 0; }
};

// scalar rows (any dim_x): a voxel per lane, a row per wavefront
inline Grid3 grid_scalar_rows(const SlabGeometry &g) { return {(unsigned)ceil_div(g.dim_x, 64), (unsigned)ceil_div(g.dim_y, 4), (unsigned)g.nz}; }
// quad rows: a quad per lane, rows_per_wg rows per workgroup (4: a row per wavefront; 8: two, the one-frame kernel)
inline Grid3 grid_quad_rows(const SlabGeometry &g, int rows_per_wg)
{
    return {(unsigned)ceil_div(g.xgroups(4), 64), (unsigned)ceil_div(g.dim_y, rows_per_wg), (unsigned)g.nz};
}
// flat: a quad per lane over the slice's linear view, a 256-voxel chunk per wavefront (also the pass that recomputes the summary)
inline Grid3 grid_flat(const SlabGeometry &g) { return {(unsigned)ceil_div(g.chunks_per_slice, 4), 1u, (unsigned)g.nz}; }
inline Grid3 grid_recompute_flags(const SlabGeometry &g) { return grid_flat(g); }

// bricks: a brick per wavefront, `blocks` workgroups of four bricks per slice group; the class table that goes with the grid
// has one byte per wavefront, padding of the last workgroup included
inline int brick_blocks(const SlabGeometry &g) { return ceil_div(g.brick_groups * g.bricks_per_group, 4); }
struct BrickGrid { Grid3 grid; size_t class_elems; };
inline BrickGrid brick_grid(int blocks, int slice_groups)
{
    return {{(unsigned)blocks, 1u, (unsigned)slice_groups}, (size_t)blocks * (size_t)slice_groups * 4};
}
inline BrickGrid brick_grid(const SlabGeometry &g) { return brick_grid(brick_blocks(g), g.nz_groups); }

// grid-stride passes of 256 lanes, 2048 workgroups at most: over the summary words (forget_runs, summary_stats) and over the
// slab's quads (fill_grid, never empty)
constexpr size_t kStridePassBlocks = 256 * 8;
inline Grid3 grid_summary_words(const SlabGeometry &g) { return {(unsigned)std::min((g.n_flags + 255) / 256, kStridePassBlocks), 1u, 1u}; }
inline Grid3 grid_fill(const SlabGeometry &g)
{
    return {(unsigned)std::max<size_t>(std::min(((size_t)g.n_vox / 4 + 255) / 256, kStridePassBlocks), 1), 1u, 1u};
}

// depth_tile_summary: a wavefront per strip of 64 pixels of a tile row (64 / tile tiles), `frames` images in y
inline Grid3 grid_tile_strips(int tiles_w, int tiles_h, int tile, int frames)
{
    const int strips = ceil_div(tiles_w, 64 / tile) * tiles_h;
    return {(unsigned)ceil_div(strips, 4), (unsigned)frames, 1u};
}

// ---- the brick work list -------------------------------------------------------------------------------------------
// Constants of the kernels (tsdf_multiframe.hip.h), restated; tsdf_capi.hip checks that they agree.
constexpr int kListBuckets = 64;
constexpr int kSuperBX = 4, kSuperBY = 2, kSuperBZ = 1;
constexpr int kSuperBricks = kSuperBX * kSuperBY * kSuperBZ;

// The sub-list (bucket) of super-brick `id` = (sx, sy, sz): workgroup j of integrate_brick_list takes its entries from sub-list
// j % kListBuckets, and workgroups are dealt to the eight XCDs round robin by their index, so sub-list b is served by XCD b % 8.
// wedge_mode 0 (what ships): a multiplicative hash of the index -- every sub-list, and with it every XCD, samples the whole
// volume: the sub-lists run dry together, but every XCD's L2 ends up fetching every depth frame of the launch (32 x 1.2 MB; an
// XCD has 4 MB).  wedge_mode 1 .. 3 (measurement build only, TSDF_WEDGE_MODE): the low three bits -- the XCD -- come from WHERE
// the super-brick lies in the image: its centre's row under the base camera, in stripes of 16 (mode 3: 8) pixels dealt round
// robin (a stripe is a wedge of the volume through the camera centre, so under any pose of the launch it projects onto a compact
// part of the image); modes 2 and 3 rotate the stripe -> XCD map by three every four super-bricks along x, so that the image's top
// and bottom rows -- where the bricks that straddle the border sit -- go round all XCDs.  Measured, round 4, same box, S-surf 512^3:
// the Integrate kernel's measured traffic 908 -> 558 / 599 / 692 MB per launch (modes 1 / 2 / 3: the depth frames are no longer
// fetched into all eight L2s) but 0.0256 -> 0.0305 / 0.0283 / 0.0276 ms per frame (4.5 - 5.0 resident wavefronts per SIMD instead
// of 5.6: the XCDs' shares of the per-voxel work are no longer alike, and the launch is bound by instruction issue, not by
// bytes); the fr3 trajectory 4.15 -> 3.82 GB, 0.1498 -> 0.1507.  Integer arithmetic only: the host sizes the sub-lists with the
// same function (work_list_layout).
TSDF_HOST_DEVICE inline unsigned int list_bucket(const unsigned int id, const int sx, const int sy, const int sz, const int wedge_mode,
                                                 const int wedge_oy, const int wedge_oz, const int super_h, const int super_d, const int fy_px)
{
    const unsigned int h = id * 2654435761u;
    if (wedge_mode == 0) return h >> 26;
    const int yc = wedge_oy + (2 * sy + 1) * super_h / 2;
    int zc = wedge_oz + (2 * sz + 1) * super_d / 2;
    if (zc < 1) zc = 1;
    int t = (yc * 256) / zc;                             // 256 * tan of the elevation; |yc| < 2^19
    t = t > 65536 ? 65536 : (t < -65536 ? -65536 : t);   // (a tangent beyond 256 is outside any image; keeps the product below 2^31)
    const int stripe = (t * fy_px) >> (wedge_mode == 3 ? 11 : 12);       // rows / 16 or / 8 (arithmetic shift: floor)
    const int rot = wedge_mode >= 2 ? 3 * (sx >> 2) : 0;
    return ((h >> 29) << 3) | ((unsigned int)(stripe + rot) & 7u);
}

// The list of a slab: super-bricks of kSuperBX x kSuperBY x kSuperBZ bricks along x, row groups and slice groups; the six
// integers list_bucket reads (the base camera's position in voxel units relative to voxel (0, 0, z_begin) of the slab, clamped
// and rounded -- the key only has to be the same on host and device --, the super-brick's height and depth in voxels, the focal
// length in pixels); and the capacity: a sub-list must hold every brick of every super-brick list_bucket deals to it, counted
// exactly, in the index order of classify_brick_list.
struct WorkListLayout {
    int nsx = 0, nsy = 0, nsz = 0;
    int wedge_mode = 0, wedge_oy = 0, wedge_oz = 0, super_h = 0, super_d = 0, fy_px = 1;
    int64_t n_super = 0;         // nsx * nsy * nsz
    int64_t bucket_supers = 0;   // most super-bricks in one sub-list
    int64_t bucket_cap = 0;      // entries per sub-list: bucket_supers * kSuperBricks
    int64_t total = 0;           // entries of the list: bucket_cap * kListBuckets
    bool fits = true;            // the list's 32-bit index holds `total` and the grid's padding
};

constexpr int64_t kMaxWorkListEntries = 0x7fffffffll - 1024;

// capacity from the fullest sub-list
inline void work_list_capacity(WorkListLayout &w, int64_t bucket_supers)
{
    w.bucket_supers = bucket_supers;
    w.bucket_cap = bucket_supers * kSuperBricks;
    w.total = w.bucket_cap * kListBuckets;
    w.fits = w.total <= kMaxWorkListEntries;
}

inline WorkListLayout work_list_layout(const tsdf_config &c, const SlabGeometry &g, int wedge_mode)
{
    WorkListLayout w;
    if (g.brick_q <= 0) return w;      // no brick view, no list
    w.nsx = ceil_div(g.bricks_per_group, kSuperBX);
    w.nsy = ceil_div(g.brick_groups, kSuperBY);
    w.nsz = ceil_div(g.nz_groups, kSuperBZ);
    w.super_h = kSuperBY * g.brick_r;
    w.super_d = kSuperBZ * g.brick_s;
    w.wedge_oy = (int)std::lround(std::fmax(-30000.0, std::fmin(30000.0, (double)c.origin[1] / c.voxel_size)));
    w.wedge_oz = (int)std::lround(std::fmax(-30000.0, std::fmin(30000.0, (double)c.origin[2] / c.voxel_size + c.z_begin)));
    w.fy_px = (int)std::lround(std::fmax(1.0, std::fmin(16000.0, std::fabs((double)c.cam_K[4]))));
    w.wedge_mode = (!(c.voxel_size > 0) || std::isnan(c.origin[1]) || std::isnan(c.origin[2])) ? 0 : wedge_mode;
    w.n_super = (int64_t)w.nsx * w.nsy * w.nsz;
    // (the fullest sub-list holds at least the mean: a list that cannot fit is refused without being counted)
    work_list_capacity(w, (w.n_super + kListBuckets - 1) / kListBuckets);
    if (!w.fits) return w;
    int64_t per[kListBuckets] = {};
    for (int64_t id = 0; id < w.n_super; ++id) {      // slice groups fastest, then x, then y
        const int sz = (int)(id % w.nsz), sx = (int)((id / w.nsz) % w.nsx), sy = (int)((id / w.nsz) / w.nsx);
        ++per[list_bucket((unsigned int)id, sx, sy, sz, w.wedge_mode, w.wedge_oy, w.wedge_oz, w.super_h, w.super_d, w.fy_px)];
    }
    work_list_capacity(w, *std::max_element(per, per + kListBuckets));
    return w;
}

// classify_brick_list: a wavefront per super-brick
inline Grid3 grid_classify_list(const WorkListLayout &w) { return {(unsigned)((w.n_super + 3) / 4), 1u, 1u}; }
// integrate_brick_list: a wavefront per entry, sized for the worst case: the front groups and the back groups of every sub-list
inline Grid3 grid_brick_list(const WorkListLayout &w) { return {(unsigned)(((w.bucket_cap + 3) / 4 + 1) * kListBuckets), 1u, 1u}; }

// ---- the summary duty ----------------------------------------------------------------------------------------------
// What a launch that writes weights keeps of the summary words (host_derive.h, "the summary word"):
//   Nothing   the scalar kernel and the measurement build's kernels without a summary: the words are zeroed ahead of them
//   Bits      bits 0 and 1: the fused, flat, brick and batched kernels, the ladder's summary kernels, variant 11; a kernel that
//             meets a run does not load the segment's weights, so the runs are forgotten ahead of them (forget_runs)
//   Runs      bits 0 and 1 and the weight runs: integrate_tile alone
enum class Keeps { Nothing, Bits, Runs };
enum class SummaryAction { None, Zero, ForgetRuns };   // what to queue ahead of the launch

// What the host knows of a handle's words without reading them.  The words are zeroed only when they are not known to be zero
// and the runs forgotten only when one may be set; every transition that drops an action errs to the cautious side.
struct SummaryRecord {
    bool known_zero = false;   // every word is zero
    bool runs_maybe = false;   // some word may carry a run (bit 2 and a count)

    SummaryAction before_launch(Keeps keeps)
    {
        if (keeps == Keeps::Nothing) {
            if (known_zero) return SummaryAction::None;
            known_zero = true;
            runs_maybe = false;
            return SummaryAction::Zero;
        }
        const bool forget = keeps == Keeps::Bits && runs_maybe;
        known_zero = false;
        runs_maybe = keeps == Keeps::Runs;
        return forget ? SummaryAction::ForgetRuns : SummaryAction::None;
    }
    void after_fill() { known_zero = false; runs_maybe = true; }      // every word is kSummaryFresh: the count 0
    void after_rebuild() { known_zero = false; runs_maybe = true; }   // recompute_flags finds the runs the arrays hold
};

// ---- the kernel of a one-frame launch ------------------------------------------------------------------------------
// Scalar: rows of no multiple of 4 voxels, or the scalar variant.  MaskedBricks: a masked frame whose launch is classified
// (classify_one_frame), given tile tables that fit and a brick view, row-mapped or flat.  Otherwise FlatSingle (rows of no
// multiple of 256 voxels: the fused kernel with one frame) or Tile (integrate_tile).  With what the choice keeps of the words.
enum class OneFrameKernel { Scalar, FlatSingle, MaskedBricks, Tile };
struct OneFrame { OneFrameKernel kernel; Keeps keeps; };

inline OneFrame one_frame(const SlabGeometry &g, const Variant &var, bool masked, bool tiles_fit)
{
    if (!g.quad_rows || var.scalar) return {OneFrameKernel::Scalar, Keeps::Nothing};
    if (masked && classify_one_frame(var.classify, g.n_vox) && tiles_fit && g.brick_q > 0) return {OneFrameKernel::MaskedBricks, Keeps::Bits};
    if (g.flat) return {OneFrameKernel::FlatSingle, Keeps::Bits};
    return {OneFrameKernel::Tile, Keeps::Runs};
}

}  // namespace tsdf_host
