// host_derive.h -- what the host derives from a configuration and a pose before a launch: the wavefront brick, the depth tile
// edge and the guards / margins that make the kernels' shortcuts exact ("Why each shortcut is exact").
// Plain C++ (no HIP, no device types): tsdf_capi.hip includes it for the product, and the CPU sanitizer run compiles it by
// itself with -fsanitize=address,undefined (tests/test_sanitizers.py).
// Also the launch policy: what a kernel variant means, tile tables, pipelining, classification, the sweep's cache window, batches.
// And the encoding of the summary word with its transition under a one-frame launch, which the kernels share (the one place
// where a function here carries the host / device marker, and only when the HIP compiler reads it).
// What a launch's grids, class table, work list and table offsets follow from -- a slab's geometry -- is in launch_geometry.h,
// which builds on this file.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>

#include "tsdf_hip.h"

namespace tsdf_host {

// The wavefront brick of classified launches: q quads (4q voxels) of r rows of s slices, q * r * s <= 64 lanes, q a
// divisor of the row's quads.  A brick is classified as a whole, so what counts is how tightly its box projects
// (few depth tiles, a short range of camera depths) and how it coalesces (16q-byte row pieces).
inline bool brick_shape_ok(const tsdf_config &c, int q, int r, int s)
{
    // (the last condition: a lane's byte offset within its brick is a 32-bit number in the kernels)
    return c.dim_x % 4 == 0 && q >= 1 && r >= 1 && s >= 1 && q * r * s <= 64 && (c.dim_x / 4) % q == 0 &&
           (long long)s * c.dim_x * c.dim_y < (1ll << 30);
}

// The library's choice: the shape that lets the fewest bricks touch a surface band.  A brick of X x Y x Z voxels is
// claimed unless the band (about 10 voxels thick) crosses its box grown by the slack of the depth tiles it is tested
// against (about 8 voxels either way in x and y at the usual 1 - 2 pixels per voxel), so the share of per-voxel
// bricks goes like (X + 8)(Y + 8)(Z + 10) / XYZ; idle lanes and row pieces under 64 bytes (q < 4) cost on top.
// Measured over shapes at 512^3 S-surf (ms per frame, fused): 2,4,8 0.0431; 2,8,4 0.0475; 4,4,4 0.0479; 4,8,2
// 0.0492; 1,8,8 0.0515; 8,8,1 0.0528; 16,4,1 0.0669 -- the same order as this cost; 200^3 @ 4 mm and the 1024^3
// trajectory agree (tools/claim_sim.py replays the claim rule on the CPU: 8 x 4 x 8 voxels leaves the
// fewest bricks undecided of eight shapes).
inline void choose_brick_default(const tsdf_config &c, int &bq, int &br, int &bs)
{
    bq = 0; br = 0; bs = 1;
    if (c.dim_x % 4 != 0) return;
    const int quads = c.dim_x / 4;
    const int nz = c.z_end - c.z_begin;
    double best = 1e300;
    for (int q = 1; q <= 64 && q <= quads; ++q) {
        if (quads % q) continue;
        for (int sl = 1; q * sl <= 64 && sl <= std::max(nz, 1); ++sl) {
            const int r = std::min(64 / (q * sl), std::max(c.dim_y, 1));
            if (!brick_shape_ok(c, q, r, sl)) continue;
            const double X = 4.0 * q, Y = r, Z = sl;
            const double cost = (X + 8.0) * (Y + 8.0) * (Z + 10.0) / (X * Y * Z) * (1.0 + 0.25 / q) * 64.0 / (q * r * sl);
            if (cost < best) { best = cost; bq = q; br = r; bs = sl; }
        }
    }
}

// Guards and margins of one frame: everything below is derived from the configuration and the frame's cam2base pose.
struct ProjectionGuards {
    float cz_margin;    // corner test of a lane's patch against the camera plane (claim 6)
    int fast_ok;        // the shared-reciprocal projection is exact for every operand this slab and pose can produce (claim 4)
    int trunc_fast;     // diff / trunc through the launch-wide refined reciprocal
    float cz_short;     // classify_patch: camera-frame z below which a box's projected corners are not trusted
    float cz_pad;       // classify_patch: widening of the z bounds (twice the error bound on cz)
    float px_margin_u, px_margin_v;   // classify_patch: widening of the projected pixel box
};

// c2b: row-major 4x4 camera-to-base pose of the frame (ref: src/tsdf.cu:142).
inline ProjectionGuards derive_projection_guards(const tsdf_config &c, const float *c2b)
{
    ProjectionGuards g;
    const double fx = c.cam_K[0], fy = c.cam_K[4], cx = c.cam_K[2], cy = c.cam_K[5];
    // The shared-reciprocal projection (tsdf_kernels.hip.h, fast_div2) is exact when no operand
    // needs div_scale's pre-scaling: bound every camera-frame coordinate of the slab by
    // sum_j |R_ij| * max|d_j| and keep it, and the intrinsics, far from the exponent limits.
    // Anything else (including NaN/inf in the pose) takes the generic IEEE-division path.
    const double ext[3] = {(double)(c.dim_x - 1) * c.voxel_size, (double)(c.dim_y - 1) * c.voxel_size,
                           (double)(c.dim_z - 1) * c.voxel_size};
    const double o[3] = {c.origin[0], c.origin[1], c.origin[2]}, t[3] = {c2b[3], c2b[7], c2b[11]};
    double dmax[3];
    for (int k = 0; k < 3; ++k) dmax[k] = std::fmax(std::fabs(o[k] - t[k]), std::fabs(o[k] + ext[k] - t[k])) * 1.001 + 1e-30;
    // rows[i][k]: coefficient of d_k in camera coordinate i (the transposed rotation: columns of the row-major pose)
    const double rows[3][3] = {{c2b[0], c2b[4], c2b[8]}, {c2b[1], c2b[5], c2b[9]}, {c2b[2], c2b[6], c2b[10]}};
    bool ok = true;
    double bz = 0;
    for (int i = 0; i < 3; ++i) {
        double b = 0;
        for (int k = 0; k < 3; ++k) b += std::fabs(rows[i][k]) * dmax[k];
        ok = ok && (b < 5.7e17);  // 2^59; false for NaN/inf
        if (i == 2) bz = b;
    }
    // rounding error of cz is < 4 ulp of bz (2.4e-7 bz): the margin is 40x that, never below 1e-17
    g.cz_margin = ok ? (float)std::fmax(1e-5 * bz, 1e-17) : 3.0e38f;
    ok = ok && std::fabs(fx) < 16384.0 && std::fabs(fy) < 16384.0 &&
         std::fabs(cx) < 1048576.0 && std::fabs(cy) < 1048576.0 &&
         (int64_t)c.im_width * c.im_height <= (1 << 24) &&   // pixel index exact in fp32
         c.im_width < (1 << 24) && c.im_height < (1 << 24);   // and its factors fit the 24-bit multiply
    g.fast_ok = ok ? 1 : 0;
    // diff / trunc through the shared reciprocal (tsdf_kernels.hip.h, fast_div_r): divisor and numerator ranges
    g.trunc_fast = (ok && c.trunc_margin >= 9.5367431640625e-07f && c.trunc_margin <= 1048576.0f &&
                    c.max_depth <= 5.7e17f) ? 1 : 0;   // 2^-20 .. 2^20; max_depth <= 2^59 (false for NaN)
    // Patch classification (tsdf_multiframe.hip.h, classify_patch).  E_k bounds how far a voxel's d_k = (o_k +
    // i*vs) - t_k, as rounded on the per-voxel path, lies from the affine function of the index (two roundings at
    // the magnitude of the coordinate, one at that of the difference); eps bounds the error of a camera-frame
    // coordinate on either path (those, through the rotation, plus five roundings at the magnitude b_i), twice.
    double bmax = 0, eps = 0;
    for (int i = 0; i < 3; ++i) {
        double b = 0, e = 0;
        for (int k = 0; k < 3; ++k) {
            const double Ek = 1.2e-7 * (std::fabs(o[k]) + ext[k] + std::fabs(t[k])) + 6e-8 * dmax[k];
            b += std::fabs(rows[i][k]) * dmax[k];
            e += std::fabs(rows[i][k]) * Ek;
        }
        bmax = std::fmax(bmax, b);
        eps = std::fmax(eps, 2.0 * (e + 3.0e-7 * b));
    }
    const bool sok = ok && bmax > 0 && eps < 1e30;
    g.cz_short = sok ? (float)(std::fmax(bmax / 64.0, eps / 3.2e-5) * 1.0001) : 3.0e38f;
    g.cz_pad = sok ? (float)(std::fmax(2.0 * eps, (double)g.cz_margin) * 1.0001) : 3.0e38f;
    // By how much the pixel box of a patch's projected corners is widened so that it holds the rounded pixel of every voxel of
    // the patch as the per-voxel path computes it:  0.5 (a pixel index is within half a pixel of its u)  +  the projection error
    // of BOTH paths for cz >= cz_short, |fx| * (eps / cz) * (1 + |t|) with eps / cz <= 3.2e-5 (eps is the sum of the two paths'
    // camera-coordinate errors, above) and |t| <= 4 (W + |cx|) / |fx| for every corner that can matter (a corner with a larger
    // tangent projects more than four image widths outside, where an error of a pixel changes nothing; cz >= bmax / 64 keeps
    // it below 1.1 pixels there)  +  1/16 for the roundings of u = fx * q + cx itself (two ulp of a number below 2^13 for such
    // corners: 2e-3).  (Round 2 carried a whole pixel of unexplained slack on top: with 8-pixel tiles that pixel decided one
    // box in twelve -- S-surf 512^3: 11.6 % -> 10.7 % of the wavefront-frames per voxel, 0.0270 -> 0.0257 ms per frame.)
    g.px_margin_u = (float)(0.5625 + 3.2e-5 * (std::fabs(fx) + 4.0 * (c.im_width + std::fabs(cx))));
    g.px_margin_v = (float)(0.5625 + 3.2e-5 * (std::fabs(fy) + 4.0 * (c.im_height + std::fabs(cy))));
    return g;
}

// ---- launch policy ------------------------------------------------------------------------------------------------
// Constants of the kernels (tsdf_multiframe.hip.h), restated; tsdf_capi.hip checks that they agree.
constexpr int kMaxFramesPerLaunch = 32;
constexpr int kTileLdsEntries = 5120;
constexpr int kFineTile = 4;
constexpr int kFineLevels = 3;

// Kernel variants (tsdf_set_kernel_variant) of the library as shipped:
//   0   default: one call = one launch of integrate_tile<2> (rows of a multiple of 256 voxels), of the flat kernel (other
//       rows of a multiple of 4 voxels) or of the scalar kernel (any other row); collected frames and frame sequences
//       (tsdf_integrate_frames_device, ..._sequence_timed) are applied up to kMaxFramesPerLaunch (32) per pass over the
//       volume -- over the brick work list when the depth tile tables earn their keep (decided per launch from the previous
//       launch's claims), else by the per-voxel fused kernel
//   3   as 0 but one launch per frame even for sequences
//   7   as 0 but never classified (the per-voxel fused kernel alone)
//   8   as 0 but always classified
//   1   the scalar kernel (any dim_x)
// Every other number belongs to the measurement build (-DTSDF_EXPERIMENTS: tsdf_experiments.hip.h, `make experiments`), which
// decodes its own (tsdf_experiments_host.hip.h, experiment_variant).
enum class Classify { Adaptive, Never, Always };

struct Variant {
    bool known = false;    // false: not a variant of this build
    bool fuses = false;    // collected frames and sequences go through the fused kernels (rows of a multiple of 4 voxels)
    bool scalar = false;   // one-frame launches run the scalar kernel whatever the row length
    Classify classify = Classify::Adaptive;
};

inline Variant decode_variant(int variant)
{
    switch (variant) {
        case 0: return {true, true, false, Classify::Adaptive};
        case 1: return {true, false, true, Classify::Adaptive};
        case 3: return {true, false, false, Classify::Adaptive};
        case 7: return {true, true, false, Classify::Never};
        case 8: return {true, true, false, Classify::Always};
        default: return {};
    }
}

inline int64_t slab_voxels(const tsdf_config &c) { return (int64_t)c.dim_x * c.dim_y * (int64_t)(c.z_end - c.z_begin); }

// Depth tile tables (tsdf_multiframe.hip.h): a sparse table of tile_levels(tw) x tile_levels(th) levels per frame, built
// only for frames of at most kMaxTableTiles tiles (larger frames are not classified).
inline int tile_levels(int n) { int l = 0; while (n > 0) { ++l; n >>= 1; } return l; }

inline size_t tile_table_elems(int tiles_w, int tiles_h)
{
    return (size_t)tile_levels(tiles_w) * tile_levels(tiles_h) * tiles_w * tiles_h;
}

constexpr int64_t kMaxTableTiles = 16384;
inline bool tiles_fit(int tiles_w, int tiles_h) { return (int64_t)tiles_w * tiles_h <= kMaxTableTiles; }
// Tiles of `edge` pixels along an image axis of n pixels (the last one may overhang the image)
inline int tiles_along(int n, int edge) { return (n + edge - 1) / edge; }

// Pixels per depth tile edge for a slab: 8 where a fused launch is long enough to repay tables four times as large (the finer
// tiles leave a fifth fewer wavefront-frames to the per-voxel path: tsdf_multiframe.hip.h), 16 otherwise and wherever the finer
// grid of tiles would not fit the table kernels.  Measured on S-surf, ms per frame with 16 / 8: 128^3 0.0044 / 0.0051 (before
// the table kernel ran 1024 threads), 200^3 0.00586 / 0.00586, 224^3 0.00642 / 0.00633, 256^3 0.00764 / 0.00741, 288^3 0.0097 /
// 0.0093, 320^3 0.0114 / 0.0106, 512^3 0.0312 / 0.0270: the finer tiles pay from about 10 M voxels.  Members of a batch share one
// table layout and keep 16.
constexpr int64_t kFineTileMinVoxels = 10000000;
inline int tile_edge(const tsdf_config &c, bool batch_member)
{
    const int64_t fine_tiles = (int64_t)tiles_along(c.im_width, 8) * tiles_along(c.im_height, 8);
    return (!batch_member && slab_voxels(c) >= kFineTileMinVoxels && fine_tiles <= kTileLdsEntries) ? 8 : 16;
}

// Fine (4-pixel) tiles beside the 8-pixel tables: where a fused launch is long enough to repay two more small table kernels and
// 1.4 MB more table per frame (tsdf_multiframe.hip.h, fine_tile_levels).
constexpr int64_t kFineLevelMinVoxels = 64000000;      // measured: 512^3 S-surf 0.0255 -> 0.0240 ms per frame, 320^3 0.0102 -> 0.0105
inline bool fine_tables(const tsdf_config &c, int tile) { return tile == 8 && slab_voxels(c) >= kFineLevelMinVoxels; }

// A launch's table slot in the frame store, in elements of two floats: kMaxFramesPerLaunch coarse sparse tables of coarse_elems
// each from element 0, then (fine) as many fine ones of fine_elems each from fine_begin; all zero when the frame's tiles do not
// fit the tables.  A frame's coarse table is f * coarse_elems into the slot, its fine one fine_begin + f * fine_elems.
struct TableSlotLayout { size_t coarse_elems, fine_begin, fine_elems, bytes; };

inline TableSlotLayout table_slot_layout(const tsdf_config &c, int tile, bool fine)
{
    const int tw = tiles_along(c.im_width, tile), th = tiles_along(c.im_height, tile);
    if (!tiles_fit(tw, th)) return {0, 0, 0, 0};
    TableSlotLayout l;
    l.coarse_elems = tile_table_elems(tw, th);
    l.fine_begin = (size_t)kMaxFramesPerLaunch * l.coarse_elems;
    l.fine_elems = fine ? (size_t)kFineLevels * kFineLevels * tiles_along(c.im_width, kFineTile) * tiles_along(c.im_height, kFineTile) : 0;
    l.bytes = (l.fine_begin + (size_t)kMaxFramesPerLaunch * l.fine_elems) * (2 * sizeof(float));
    return l;
}

// Bytes of that slot (what the frame store is asked for): 0 when the frame's tiles do not fit the tables.
inline size_t launch_table_bytes(const tsdf_config &c, int tile, bool fine) { return table_slot_layout(c, tile, fine).bytes; }

// Pipelining pays where a launch is short enough for its small pre-pass kernels to matter and the chip is not full: measured,
// same box, sequence path, pre-pass on the handle's stream / beside the previous launch: S-surf 200^3 0.00578 -> 0.00546 ms per
// frame, 320^3 0.01043 -> 0.01037, 512^3 0.02396 -> 0.02403 (the Integrate kernel runs 76 us longer beside a pre-pass that takes
// 84 us alone: its latency-bound wavefronts hold slots the Integrate kernel's would use), fr3 trajectory 1024^3 0.1460 -> 0.1458.
// So: slabs below 64 M voxels; larger ones keep one list (the second would be 134 MB at 1024^3) and one stream.
constexpr int64_t kPipelineMaxVoxels = 64000000;
inline bool pipelines(const tsdf_config &c) { return slab_voxels(c) < kPipelineMaxVoxels; }

// One-frame masked launches are classified per workgroup when the launch is large enough to repay the three small
// dependent dispatches ahead of it (tile summary, sparse table, class table: ~25 us on the stream).  Measured
// (tools/batch_time.py, instance masks over 12 % of the image): 16 x 200^3 batched 0.275 -> 0.157 ms per frame (wavefront
// bricks; 0.201 with 1024-voxel workgroup patches), one 400^3 volume 0.095 -> 0.075; but 4 x 200^3 batched 0.083 -> 0.079
// at best and one 200^3 volume 0.016 -> 0.026.
// Variant 8 classifies regardless (tests), 7 never.
constexpr int64_t kClassifyMinVoxels = 48000000;
inline bool classify_one_frame(Classify mode, int64_t launch_voxels)
{
    if (mode == Classify::Never) return false;
    return mode == Classify::Always || launch_voxels >= kClassifyMinVoxels;
}

// Fused launches (adaptive): the first launch classifies, every classifying launch counts its claims, and a launch whose
// predecessor claimed less than a tenth of its wavefront-frames goes without (the tables and the pre-pass cost more than
// that saves), with a new probe every eighth launch.
constexpr double kMinClaimFraction = 0.10;
constexpr int kProbeEvery = 8;
inline bool classify_fused(Classify mode, bool claims_known, double claim_fraction, int launches_unclassified)
{
    if (mode != Classify::Adaptive) return mode == Classify::Always;
    return !claims_known || claim_fraction >= kMinClaimFraction || launches_unclassified >= kProbeEvery - 1;
}

// Infinity Cache window of the one-frame kernel (integrate_tile, IntegrateParams::cache_lo/hi): successive launches sweep z
// in alternate directions and the last slices of each sweep, up to kWindowBytes of TSDF + weight state, are loaded and
// stored with the default cache policy (the rest streams non-temporal), so the next launch starts on lines still in the
// 256 MiB Infinity Cache.  Chosen by measurement (tools/window_sweep.py, profiles/r05_window_sweep.txt), S-band 512^3,
// ms per frame with a window of 0 / 128 / 256 / 384 / 512 / 768 / 1024 MiB: 0.3317 / 0.3242 / 0.3205 / 0.3177 / 0.3161 /
// 0.3182 / 0.3230 (forward sweeps, no window: 0.3319); loading the slices before the window with the default policy too
// was slower (0.3232 at 64-192 MiB).  A slab whose state fits the window is swept cacheable throughout.
constexpr int64_t kWindowBytes = 512ll << 20;

struct SweepWindow { int cache_lo, cache_hi; };   // slices [cache_lo, cache_hi) of the slab, in memory order

inline SweepWindow sweep_window(int nz, int dim_x, int dim_y, int64_t window_bytes, bool reverse)
{
    const int64_t slice_bytes = 8 * (int64_t)dim_x * dim_y;
    const int w = (int)std::min<int64_t>(nz, window_bytes / slice_bytes);
    return reverse ? SweepWindow{0, w} : SweepWindow{nz - w, nz};
}

// Deferral of a batch (tsdf_batch_integrate_device): collect the frame and apply 32 at a time with one fused launch per
// member -- the volumes then move once per 32 frames, but every member costs a launch with its own tile tables per flush, so
// many small members stay with the one batched launch per frame.  Fitted to tools/batch_time.py (instance masks, ms per frame,
// batched -> deferred): 1 x 200^3 0.035 -> 0.013, 4 x 200^3 0.082 -> 0.031, 16 x 200^3 0.145 -> 0.100, 2 x 400^3 0.122 -> 0.046,
// 8 x 128^3 0.059 -> 0.047; but 16 x 64^3 0.035 -> 0.070, 64 x 100^3 0.229 -> 0.307: deferred costs about 4 us per member +
// 0.8 us per M voxels, batched 20 us + 2.8.
inline bool batch_defers(int members, int64_t total_voxels) { return 2 * (int64_t)members < 10 + total_voxels / 1000000; }

// A batched launch with instance masks is classified as a one-frame launch is (classify_one_frame), and not for many small
// volumes: one tile table per object has to be built per frame (64 x 100^3: 0.231 -> 0.262 ms).
constexpr int64_t kBatchMinVoxelsPerMember = 2000000;
inline bool batch_classifies(Classify mode, int members, int64_t launch_voxels)
{
    const bool big_enough = mode == Classify::Always || launch_voxels >= (int64_t)members * kBatchMinVoxelsPerMember;
    return big_enough && classify_one_frame(mode, launch_voxels);
}

// Streams a batch's flush spreads its members' launches over (measured, 200^3 members with instance masks, ms per frame, one
// stream -> four: 16 members 0.081 -> 0.062, 8 members 0.047 -> 0.045, 4 members 0.027 -> 0.034, 2 members 0.016 -> 0.023: few
// members fill the GPU one after the other)
constexpr int kBatchSideStreams = 4;
inline int batch_lanes(int members) { return members < 8 ? 1 : kBatchSideStreams; }

// ---- the summary word --------------------------------------------------------------------------------------------
// One 32-bit word per 256-voxel row segment (tsdf_kernels.hip.h, IntegrateParams::flags).  It holds knowledge about the arrays
// that lets a load be skipped; the arrays themselves always stay current.
//   bit 0       every TSDF value of the segment is exactly 1.0f
//   bit 1       every weight of the segment is finite and >= 0
//   bit 2       every weight of the segment has the bit pattern of (float)c, c the count below (a "weight run"; implies bit 1)
//   bits 8..31  the count c, 0 <= c <= kMaxRunCount; zero whenever bit 2 is clear
// Weights on the one-frame path are counts (every update adds exactly 1.0f), so a segment that every frame so far updated
// wholly or not at all holds 256 identical integers, and the one-frame kernel takes them from the word instead of the array.
#if defined(__HIPCC__)
#define TSDF_HOST_DEVICE __host__ __device__
#else
#define TSDF_HOST_DEVICE
#endif

constexpr uint32_t kSummaryOnes = 1u, kSummarySane = 2u, kSummaryRun = 4u;
constexpr int kRunCountShift = 8;
constexpr uint32_t kMaxRunCount = (1u << 24) - 1;   // (float)c is exact, and so is c + 1, up to here
constexpr uint32_t kSummaryFresh = kSummaryOnes | kSummarySane | kSummaryRun;   // create / reset: TSDF 1, weight 0 = count 0

TSDF_HOST_DEVICE inline bool word_has_run(uint32_t word) { return (word & kSummaryRun) != 0u; }
TSDF_HOST_DEVICE inline uint32_t word_run_count(uint32_t word) { return word >> kRunCountShift; }
// bits 0 and 1 of `low` with a run of count c <= kMaxRunCount
TSDF_HOST_DEVICE inline uint32_t word_with_run(uint32_t low, uint32_t c)
{
    return (low & (kSummaryOnes | kSummarySane)) | kSummaryRun | (c << kRunCountShift);
}
// ... and without one
TSDF_HOST_DEVICE inline uint32_t word_without_run(uint32_t word) { return word & (kSummaryOnes | kSummarySane); }

// The word of a segment after a one-frame launch: `touched` = some voxel of it was updated, `all_updated` = all 256 were,
// `left_not_one` = some updated TSDF value came out != 1.0f.  An untouched segment keeps its word.  A run goes on, one higher,
// only where the whole segment was updated and the next count still fits; the weights themselves are always w + 1.0f.
TSDF_HOST_DEVICE inline uint32_t word_after_update(uint32_t word, bool touched, bool all_updated, bool left_not_one)
{
    if (!touched) return word;
    if (left_not_one) word &= ~kSummaryOnes;
    if (!word_has_run(word)) return word;
    const uint32_t c = word_run_count(word);
    if (!all_updated || c >= kMaxRunCount) return word_without_run(word);
    return word_with_run(word, c + 1u);
}

// One block carved into regions that each start on a 256-byte boundary: add(bytes) gives the next region's offset, total() the
// bytes of the block so far (the last region is not padded).
struct Regions {
    size_t add(size_t bytes) { const size_t at = (end_ + 255) / 256 * 256; end_ = at + bytes; return at; }
    size_t total() const { return end_; }
    size_t end_ = 0;
};

}  // namespace tsdf_host
