// tsdf_scan_ground.hip.h -- marking the ground of a lidar scan, in front of the camera splat of tsdf_scan.hip.h.
//
// The reference sorts a scan into a spherical image of n_rings x n_columns cells, one point per cell (ref: src/Utility.cpp:452-496,
// projectPointCloud), and calls a cell ground when the step to the cell one ring above it is nearly level (ref: :498-553,
// groundRemoval).  Both run here on the device.  All arithmetic is fp32 in the written order (NUMFLAGS); no transcendental
// function runs on the device: the angles are tables T, C, S and the slopes tlo, thi, built on the host in double and rounded
// once (scan_ground_tables.h, which also states the quadrants, their runs of columns and WHY both searches below may be
// bisections: the tests are monotone along what they search).  tests/scan_ground_spec.py restates the rule in NumPy with
// linear counts, and the kernels match it bit for bit.
//
// Cell of point i = (x, y, z):
//     h = sqrtf(x x + y y),  range = sqrtf((x x + y y) + z z)
//     no cell unless x, y, z are finite, h > 0 and range >= min_range                                (ref: :484)
//     ring   = #{r in 0 ... n_rings : z >= T[r] h} - 1;  no cell unless 0 <= ring < n_rings          (ref: :469-472, truncated rows)
//     column = (first[q] + k - 1) mod n_columns,  q the quadrant of (x, y),
//              k = #{c in the run of q : C[c] y >= S[c] x}     -- two products compared, no subtraction  (ref: :474-481)
//              (k = 0: the cell that began in the quadrant before)
// Later point wins, as in scan_splat: a 64-bit maximum per cell over (i + 1) << 32 | bits(range); 0 = empty (ref: :487-494
// overwrites in serial order).
// Pair (r, c), r < ground_rings, of the cell's point p and the point q of cell (r + 1, c):
//     -1 if either cell is empty;  d = q - p per coordinate, hd = sqrtf(dx dx + dy dy);
//     1 if dz >= tlo hd && dz <= thi hd, else 0                                                      (ref: :510-533)
// State of cell (r, c): -1 if r < ground_rings and its pair is -1; else 1 if its pair is 1, or if mark_upper and the pair
// (r - 1, c) below it is 1 (ref: :531; with the line in, the reference's ascending loop leaves exactly this: a later -1 overwrites
// the mark from below, a later 0 does not exist); else 0.  Each cell PULLS both pairs itself, nothing is pushed, so nothing races.
// Flag of point i: 2 without a cell, 1 if its cell's state is 1 (every point of the cell, not only the cell's own), else 0.
#pragma once
#include <hip/hip_runtime.h>

#include <cfloat>
#include <cstdint>

#include "tsdf_scan.hip.h"

namespace tsdfk {

constexpr int kGroundMaxRingsDev = 128;
constexpr uint32_t kGroundNoCell = 0xFFFFFFFFu;

struct ScanGround {
    int n_rings, n_columns, ground_rings, mark_upper;
    float min_range, tlo, thi;
    int first[4], len[4];          // the quadrants' runs of columns
    const float *T, *C, *S;        // n_rings + 1, n_columns, n_columns floats in HBM
};

// sT: T in LDS (at most 129 floats: every lane bisects it, seven dependent reads at 64 rings that would each be a trip to L2).
// C and S (up to 64 KiB each) stay in HBM and are served from L2: a lane reads about log2(n_columns / 4) entries of each.
__device__ __forceinline__ uint32_t ground_cell_of(const ScanGround &g, const float *sT, const float4 q, float *range_out)
{
    const float hh = q.x * q.x + q.y * q.y;
    const float h = sqrtf(hh), range = sqrtf(hh + q.z * q.z);
    *range_out = range;
    const bool finite = fabsf(q.x) <= FLT_MAX && fabsf(q.y) <= FLT_MAX && fabsf(q.z) <= FLT_MAX;
    if (!finite || !(h > 0.0f) || !(range >= g.min_range)) return kGroundNoCell;
    int lo = 0, hi = g.n_rings + 1;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (q.z >= sT[mid] * h) lo = mid + 1; else hi = mid;
    }
    const int ring = lo - 1;
    if (ring < 0 || ring >= g.n_rings) return kGroundNoCell;
    // h > 0 and finite: (x, y) has a quadrant
    const int quad = (q.x > 0.0f && q.y >= 0.0f) ? 0 : (q.x <= 0.0f && q.y > 0.0f) ? 1 : (q.x < 0.0f && q.y <= 0.0f) ? 2 : 3;
    const int first = quad == 0 ? g.first[0] : quad == 1 ? g.first[1] : quad == 2 ? g.first[2] : g.first[3];
    const int len = quad == 0 ? g.len[0] : quad == 1 ? g.len[1] : quad == 2 ? g.len[2] : g.len[3];
    lo = 0; hi = len;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        int c = first + mid;                      // first < n_columns, mid < len <= n_columns
        if (c >= g.n_columns) c -= g.n_columns;
        if (g.C[c] * q.y >= g.S[c] * q.x) lo = mid + 1; else hi = mid;
    }
    int col = first + lo - 1;                     // -1 ... 2 n_columns - 2
    if (col < 0) col += g.n_columns; else if (col >= g.n_columns) col -= g.n_columns;
    return (uint32_t)(ring * g.n_columns + col);
}

// One point per lane: its cell into cells[i] (kGroundNoCell for none) and its key into the cell's; block_counts not null: the
// workgroup's number of points with a cell into block_counts[blockIdx.x].  Every lane reaches both barriers.
__global__ __launch_bounds__(256) void ground_splat(const ScanGround g, const float4 *__restrict__ points, int64_t n_points,
                                                    unsigned long long *__restrict__ keys, uint32_t *__restrict__ cells,
                                                    uint32_t *__restrict__ block_counts)
{
    __shared__ float sT[kGroundMaxRingsDev + 1];
    if ((int)threadIdx.x <= g.n_rings && threadIdx.x <= kGroundMaxRingsDev) sT[threadIdx.x] = g.T[threadIdx.x];
    __syncthreads();
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    uint32_t cell = kGroundNoCell;
    if (i < n_points) {
        float range;
        cell = ground_cell_of(g, sT, points[i], &range);
        cells[i] = cell;
        if (cell != kGroundNoCell)
            atomicMax(&keys[cell], ((unsigned long long)(i + 1) << 32) | (unsigned long long)__float_as_uint(range));
    }
    if (block_counts) {
        const int n = __syncthreads_count(cell != kGroundNoCell ? 1 : 0);
        if (threadIdx.x == 0) block_counts[blockIdx.x] = (uint32_t)n;
    }
}

// -1, 0 or 1 for the pair of cells (r, c) and (r + 1, c); r + 1 < n_rings.  A key whose index is not one of this scan's points
// (the key image is all zero between scans, so there is none) counts as empty rather than being followed.
__device__ __forceinline__ int ground_pair(const ScanGround &g, const unsigned long long *__restrict__ keys,
                                           const float4 *__restrict__ points, int64_t n_points, int r, int c)
{
    const unsigned long long kl = keys[(size_t)r * g.n_columns + c], ku = keys[(size_t)(r + 1) * g.n_columns + c];
    const int64_t il = (int64_t)(kl >> 32) - 1, iu = (int64_t)(ku >> 32) - 1;
    if (il < 0 || iu < 0 || il >= n_points || iu >= n_points) return -1;
    const float4 p = points[il], q = points[iu];
    const float dx = q.x - p.x, dy = q.y - p.y, dz = q.z - p.z;
    const float hd = sqrtf(dx * dx + dy * dy);
    return (dz >= g.tlo * hd && dz <= g.thi * hd) ? 1 : 0;
}

// One cell per lane, lanes along the columns, blockIdx.y the ring: the cell's state into state[], its point's index (-1 for
// none) into winner[] where asked for, and -- block_counts not null -- the workgroup's occupied cells and ground cells into
// block_counts[2 b], [2 b + 1], b = blockIdx.y * gridDim.x + blockIdx.x.  The keys are only read: a workgroup reads the rows
// above and below its own, so they cannot be cleared here; the host clears them behind this kernel.
__global__ __launch_bounds__(256) void ground_mark(const ScanGround g, const unsigned long long *__restrict__ keys,
                                                   const float4 *__restrict__ points, int64_t n_points, int8_t *__restrict__ state,
                                                   int32_t *__restrict__ winner, uint32_t *__restrict__ block_counts)
{
    const int c = (int)(blockIdx.x * 256 + threadIdx.x), r = (int)blockIdx.y;
    bool occupied = false, ground = false;
    if (c < g.n_columns) {
        const size_t cell = (size_t)r * g.n_columns + c;
        const unsigned long long key = keys[cell];
        occupied = key != 0ull;
        const int own = r < g.ground_rings ? ground_pair(g, keys, points, n_points, r, c) : 0;
        const int below = (g.mark_upper && r >= 1 && r - 1 < g.ground_rings) ? ground_pair(g, keys, points, n_points, r - 1, c) : 0;
        const int st = own < 0 ? -1 : (own == 1 || below == 1) ? 1 : 0;
        state[cell] = (int8_t)st;
        if (winner) winner[cell] = (int32_t)(key >> 32) - 1;
        ground = st == 1;
    }
    if (block_counts) {
        const int n_occ = __syncthreads_count(occupied ? 1 : 0);
        const int n_gr = __syncthreads_count(ground ? 1 : 0);
        if (threadIdx.x == 0) {
            const size_t b = (size_t)blockIdx.y * gridDim.x + blockIdx.x;
            block_counts[2 * b] = (uint32_t)n_occ;
            block_counts[2 * b + 1] = (uint32_t)n_gr;
        }
    }
}

// One point per lane: its flag into flags[] where asked for, the workgroup's number of ground points into
// block_counts[blockIdx.x] where asked for.
__global__ __launch_bounds__(256) void ground_flags(const uint32_t *__restrict__ cells, const int8_t *__restrict__ state, int64_t n_points,
                                                    uint8_t *__restrict__ flags, uint32_t *__restrict__ block_counts)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    bool ground = false;
    if (i < n_points) {
        const uint32_t cell = cells[i];
        ground = cell != kGroundNoCell && state[cell] == 1;
        if (flags) flags[i] = cell == kGroundNoCell ? 2 : ground ? 1 : 0;
    }
    if (block_counts) {
        const int n = __syncthreads_count(ground ? 1 : 0);
        if (threadIdx.x == 0) block_counts[blockIdx.x] = (uint32_t)n;
    }
}

// scan_splat with one test in front: only_ground == 0 skips a point whose flag is 1, only_ground != 0 one whose flag is not.
// A kept point keeps its index i in its key, so "later wins" among the kept points is what it is among all of them.
// block_counts not null: the workgroup's number of kept points into block_counts[blockIdx.x].
__global__ __launch_bounds__(256) void scan_splat_select(const ScanProjection p, const float4 *__restrict__ points, int64_t n_points,
                                                         unsigned long long *__restrict__ keys, const uint32_t *__restrict__ cells,
                                                         const int8_t *__restrict__ state, int only_ground,
                                                         uint32_t *__restrict__ block_counts)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    bool keep = false;
    if (i < n_points) {
        const uint32_t cell = cells[i];
        const bool ground = cell != kGroundNoCell && state[cell] == 1;
        keep = ground == (only_ground != 0);
        if (keep) scan_splat_point(p, points[i], i, keys);
    }
    if (block_counts) {
        const int n = __syncthreads_count(keep ? 1 : 0);
        if (threadIdx.x == 0) block_counts[blockIdx.x] = (uint32_t)n;
    }
}

}  // namespace tsdfk
