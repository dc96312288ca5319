// tsdf_align.hip.h -- registration of one fused volume against another (tsdf_align_volume, tsdf_align_system): the rigid motion
// that takes the destination's base frame to the source's, estimated from the two signed-distance fields themselves (direct
// SDF-to-SDF alignment), so that tsdf_fuse_volume_at can merge at a pose the volumes' own base2world do not give: a duplicate
// object fused from another stretch of the trajectory carries that stretch's drift, a moved object a stale pose.
//
// THE RULE.  Per-voxel arithmetic is float32 in the order written (the library builds with -ffp-contract=off and IEEE
// division, csrc/Makefile NUMFLAGS), so tests/align_spec.py, which restates it in float32 NumPy, makes every per-voxel decision
// and every per-pair term bit for bit as the device does; sums and the solve are double.  A constant changed here is changed
// there and in DESIGN.md ("N11") as well.
//
//   Pose      M, 3 x 4 double, takes destination base coordinates to source base coordinates.  It starts from the float32
//             entries of the caller's guess_dst2src (the first three rows, taken as given: rigidity is the caller's duty), or,
//             with no guess, from the matrix tsdf_fuse_volume composes: float32 multiply_matrix(base2world_src_inv,
//             base2world_dst) (tsdf_fuse_pose_default).  The kernel reads Rm = (float)M_R, tm = (float)M_t (TrackState).
//   Lattice   level l, s = 2^l: the destination voxels with x_i % s == 0 on every axis, ceil(dim_i / s) points per axis.
//   Candidate with t_d, w_d the destination's values at the lattice voxel:  w_d > weight_thresh && fabsf(t_d) < 1.0f (a NaN
//             fails).  Only candidates touch the source.
//   Position  p_i = origin_dst_i + (float)x_i * vs_dst;  q_i = ((Rm_i0 * p_0 + Rm_i1 * p_1) + Rm_i2 * p_2) + tm_i;
//             g_i = (q_i - origin_src_i) / vs_src.
//   Cell      inside iff every g_i >= 0.0f && g_i < (float)(dim_src_i - 1).  j_i = (int)floorf(g_i), f_i = g_i - (float)j_i; the
//             upper corner is always j_i + 1 (unlike the merge rule there is no collapse onto the lattice: a collapsed cell has
//             a zero difference, and two identical grids would have a zero gradient everywhere).  Every index is in bounds by
//             construction; the source needs every dim >= 2.
//   Sample    the 8 corners c_abc (a along x); all 8 corner weights must be > weight_thresh.
//             d_bc = c_1bc - c_0bc;  a_bc = c_0bc + f_0 * d_bc;  b_c = a_0c + f_1 * (a_1c - a_0c);  F = b_0 + f_2 * (b_1 - b_0)
//             (fuse_sample's order).   Gradient, in source grid units, from the same corners:
//             e_c = d_0c + f_1 * (d_1c - d_0c);  G_0 = e_0 + f_2 * (e_1 - e_0);
//             h_c = a_1c - a_0c;                 G_1 = h_0 + f_2 * (h_1 - h_0);      G_2 = b_1 - b_0.
//   Pair      on the host, float32: ratio = trunc_src / trunc_dst, gscale = ratio / vs_src.
//             t = F * ratio;  r = t - t_d;  n_i = G_i * gscale  (destination truncation units per metre).
//             Rejected unless F is finite, fabsf(t) < 1.0f, fabsf(r) <= resid_thresh, every n_i is finite and
//             ((n_0 * n_0 + n_1 * n_1) + n_2 * n_2) > 0 (a NaN rejects).
//             J = (q x n, n) = (q1*n2 - q2*n1, q2*n0 - q0*n2, q0*n1 - q1*n0, n0, n1, n2): track_pair_at's order with P := q,
//             nm := n.  A step (w, tau) moves q to q + w x q + tau, so r changes by J . (w, tau).
//   Terms, system, solve, levels, status: exactly tsdf_track.hip.h's.  Per pair, in float32: J_a * J_b for a <= b (21), J_a * r
//             (6), r * r, and 1; the system is their double sum.  Cholesky with the 1e-12 * max diagonal pivot test;
//             M <- [Rodrigues(w) | tau] * M; a level ends when |w| < eps_rot and |tau| < eps_trans.  Levels n_levels-1 .. 0,
//             iters[l] iterations each.  status 2 = lost (fewer pairs than min_pairs, or a failed pivot), else 0 when the last
//             level that ran ended by the test, else 1.  The result's dst2src is each entry of M rounded to float32 with last
//             row 0 0 0 1; on a lost run it is the starting matrix's own bits.  pairs and rmse = sqrt(sum r^2 / pairs) are
//             those of the last iteration that ran.
//
// LIMITS.  The residual exists only where both fields are inside their truncation bands, so the basin is about one truncation
// distance of surface displacement; the coarse levels subsample the lattice, they do not widen the basin.  A caller with a
// larger error starts from a better guess (for instance the two centroids of tsdf_extent_metric).  The library decides
// nothing: whether the result is trusted is the caller's call from pairs, rmse and a following write = 0 merge.  Labels and
// colours are not read.  The defaults (tsdf_align_params_default) are choices, not measurements.
//
// MAPPING.  align_pairs: one lane per lattice point.  A wavefront takes a tile of 16 x 4 lattice points of one lattice slice
// (16 s x 4 s voxels): at s = 1 its destination loads are four whole 64-byte row pieces, and its gathers -- two x-neighbours in
// two rows of two slices per lane -- fall into about 5 source rows of 2 or 3 slices at the rotations inside the basin and meet
// in L1 / L2 (fuse_volume's 32 x 8 voxel tile holds four voxels per lane; with one lattice point per lane the same 2:1 shape in
// rows would be 4 rows of 64 bytes, and that is this tile).  Tiles are numbered x fastest, then y, then z; lane index =
// tile * 64 + lane, walked by a fixed-order grid-stride loop over at most kAlignMaxBlocks 256-lane workgroups (four
// consecutive tiles each).  The candidate test is made on the destination's two loads; a wavefront with no candidate is skipped
// by ballot, and the 16 source gathers are issued only under the test: free space and unobserved voxels cost two loads and a
// compare.  The reduction is track_pairs' own: 29 double accumulators, __shfl_xor over 64 lanes, the four waves through LDS in
// wave order, one partial row per workgroup by plain stores.  No atomics: equal inputs give equal bits.  track_init and
// track_solve (tsdf_track.hip.h) hold and advance the state; the finished / lost flags let the host queue every iteration of
// every level without a round trip.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "tsdf_track.hip.h"

namespace tsdfk {

constexpr int kAlignMaxBlocks = 256;     // partial rows of one pass
constexpr int kAlignTileX = 16, kAlignTileY = 4;   // lattice points of a wavefront's tile (64 lanes)
static_assert(kAlignTileX * kAlignTileY == 64, "a tile is one wavefront");

struct AlignPairsParams {
    const float *dt, *dw;        // destination TSDF and weight
    const float *st, *sw;        // source
    const TrackState *state;
    double *partials;            // gridDim.x rows of kTrackTerms
    float od[3], os[3];          // origins
    float vsd, vss;              // voxel sizes
    float hi[3];                 // (float)(dim_src_i - 1)
    int sdim[3], ddim[3];
    int ln[3];                   // lattice points per axis
    int tiles_x, tiles_y;        // tiles per lattice row and column
    unsigned n_lanes;            // tiles * 64 (< 2^31: checked on the host)
    int s, level;
    float ratio, gscale, wthr, rthr;
};

// The pair of the candidate at destination position p (metres) with destination value td, or false.
__device__ __forceinline__ bool align_pair_at(const AlignPairsParams &P, const float Rm[9], const float tm[3], const float p[3],
                                              float td, float J[6], float &r)
{
    float q[3], g[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        q[a] = ((Rm[3 * a] * p[0] + Rm[3 * a + 1] * p[1]) + Rm[3 * a + 2] * p[2]) + tm[a];
        g[a] = (q[a] - P.os[a]) / P.vss;
    }
    if (!(g[0] >= 0.0f && g[0] < P.hi[0] && g[1] >= 0.0f && g[1] < P.hi[1] && g[2] >= 0.0f && g[2] < P.hi[2])) return false;
    const int j0 = (int)floorf(g[0]), j1 = (int)floorf(g[1]), j2 = (int)floorf(g[2]);
    const float f0 = g[0] - (float)j0, f1 = g[1] - (float)j1, f2 = g[2] - (float)j2;
    const int64_t sy = P.sdim[0], sz = (int64_t)P.sdim[0] * P.sdim[1];
    const int64_t r00 = j2 * sz + j1 * sy + j0, r10 = r00 + sy, r01 = r00 + sz, r11 = r01 + sy;
    const float *t = P.st, *w = P.sw;
    const float w000 = w[r00], w100 = w[r00 + 1], w010 = w[r10], w110 = w[r10 + 1];
    const float w001 = w[r01], w101 = w[r01 + 1], w011 = w[r11], w111 = w[r11 + 1];
    const float c000 = t[r00], c100 = t[r00 + 1], c010 = t[r10], c110 = t[r10 + 1];
    const float c001 = t[r01], c101 = t[r01 + 1], c011 = t[r11], c111 = t[r11 + 1];
    const float thr = P.wthr;
    if (!(w000 > thr && w100 > thr && w010 > thr && w110 > thr && w001 > thr && w101 > thr && w011 > thr && w111 > thr)) return false;
    const float d00 = c100 - c000, d10 = c110 - c010, d01 = c101 - c001, d11 = c111 - c011;
    const float a00 = c000 + f0 * d00, a10 = c010 + f0 * d10, a01 = c001 + f0 * d01, a11 = c011 + f0 * d11;
    const float h0 = a10 - a00, h1 = a11 - a01;
    const float b0 = a00 + f1 * h0, b1 = a01 + f1 * h1;
    const float G2 = b1 - b0;
    const float F = b0 + f2 * G2;
    const float e0 = d00 + f1 * (d10 - d00), e1 = d01 + f1 * (d11 - d01);
    const float G0 = e0 + f2 * (e1 - e0);
    const float G1 = h0 + f2 * (h1 - h0);
    const float tt = F * P.ratio;
    r = tt - td;
    const float n[3] = {G0 * P.gscale, G1 * P.gscale, G2 * P.gscale};
    if (!(__builtin_isfinite(F) && fabsf(tt) < 1.0f && fabsf(r) <= P.rthr)) return false;
    if (!(__builtin_isfinite(n[0]) && __builtin_isfinite(n[1]) && __builtin_isfinite(n[2]))) return false;
    if (!(((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2]) > 0.0f)) return false;
    J[0] = q[1] * n[2] - q[2] * n[1];
    J[1] = q[2] * n[0] - q[0] * n[2];
    J[2] = q[0] * n[1] - q[1] * n[0];
    J[3] = n[0]; J[4] = n[1]; J[5] = n[2];
    return true;
}

__global__ __launch_bounds__(256) void align_pairs(AlignPairsParams P)
{
    const TrackState *st = P.state;
    if (st->lost || st->done[P.level]) return;
    float Rm[9], tm[3];
#pragma unroll
    for (int k = 0; k < 9; ++k) Rm[k] = st->Rm[k];
#pragma unroll
    for (int k = 0; k < 3; ++k) tm[k] = st->tm[k];
    double acc[kTrackTerms];
#pragma unroll
    for (int k = 0; k < kTrackTerms; ++k) acc[k] = 0.0;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    // n_lanes is a multiple of 64 and a wavefront's lanes share their tile: the trip count is uniform over the wavefront
    for (unsigned idx = blockIdx.x * 256 + threadIdx.x; idx < P.n_lanes; idx += gridDim.x * 256) {
        const unsigned tile = idx >> 6;
        const unsigned trow = tile / (unsigned)P.tiles_x;
        const int lz = (int)(trow / (unsigned)P.tiles_y);
        const int lx = (int)(tile - trow * (unsigned)P.tiles_x) * kAlignTileX + lane % kAlignTileX;
        const int ly = (int)(trow - (unsigned)lz * (unsigned)P.tiles_y) * kAlignTileY + lane / kAlignTileX;
        const int x = lx * P.s, y = ly * P.s, z = lz * P.s;
        float td = 1.0f, wd = 0.0f;
        if (lx < P.ln[0] && ly < P.ln[1]) {      // lz < ln[2] by the tile count
            const int64_t at = ((int64_t)z * P.ddim[1] + y) * P.ddim[0] + x;
            td = P.dt[at];
            wd = P.dw[at];
        }
        const bool cand = wd > P.wthr && fabsf(td) < 1.0f;
        if (__ballot(cand) == 0) continue;
        if (!cand) continue;
        const float p[3] = {P.od[0] + (float)x * P.vsd, P.od[1] + (float)y * P.vsd, P.od[2] + (float)z * P.vsd};
        float J[6], r;
        if (!align_pair_at(P, Rm, tm, p, td, J, r)) continue;
        int k = 0;
#pragma unroll
        for (int a = 0; a < 6; ++a)
#pragma unroll
            for (int b = a; b < 6; ++b) acc[k++] += (double)(J[a] * J[b]);
#pragma unroll
        for (int a = 0; a < 6; ++a) acc[21 + a] += (double)(J[a] * r);
        acc[27] += (double)(r * r);
        acc[28] += 1.0;
    }
    __shared__ double lds[4][kTrackTerms];
#pragma unroll
    for (int k = 0; k < kTrackTerms; ++k) {
        const double x = track_wave_sum(acc[k]);
        if (lane == 0) lds[wave][k] = x;
    }
    __syncthreads();
    if (threadIdx.x < kTrackTerms) {
        const int k = threadIdx.x;
        P.partials[(int64_t)blockIdx.x * kTrackTerms + k] = ((lds[0][k] + lds[1][k]) + lds[2][k]) + lds[3][k];
    }
}

}  // namespace tsdfk
