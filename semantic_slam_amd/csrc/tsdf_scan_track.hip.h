// tsdf_scan_track.hip.h -- tracking a lidar scan against the fused volume (tsdf_scan_track, tsdf_scan_track_system): the rigid
// motion that takes the scanner's frame to the world, estimated from the scan's points and the signed-distance field itself
// (point to signed distance).  Every point, taken through the pose estimate, should land where the field is zero: the
// trilinearly sampled value is the residual, its gradient the normal.  No image is made: the whole revolution takes part,
// not only the few percent of it that fall into the camera's view.
//
// THE RULE.  Per-point arithmetic is float32 in the order written (the library builds with -ffp-contract=off and IEEE
// division, csrc/Makefile NUMFLAGS), so tests/scan_track_spec.py, which restates it in float32 NumPy, makes every per-point
// decision and every per-pair term bit for bit as the device does; sums and the solve are double.  A constant changed here is
// changed there and in DESIGN.md ("N17") as well.
//
//   Pose      M, 3 x 4 double, takes scanner coordinates to the volume's base coordinates.  It starts from the float32 entries
//             of multiply_matrix(base2world_inv, guess_velo2world) (the order of tsdf_fuse_pose_default's product), where only
//             the first three rows of the guess are read (its last row is taken as 0 0 0 1; rigidity is the caller's duty).
//             The kernel reads Rm = (float)M_R, tm = (float)M_t (TrackState).
//   Selection level l, s = 2^l: the points with index % s == 0, in scan order (ceil(n_points / s) of them).  A point (x, y, z,
//             intensity; the intensity is read with the point and ignored) is a candidate when x, y and z are finite and
//             rmin2 <= ((x * x + y * y) + z * z) <= rmax2, with rmin2 = min_range_m * min_range_m and rmax2 = max_range_m *
//             max_range_m (float32 products, made once on the host), and, with flags, flags[index] != drop_flag.  Every
//             comparison is written positively: a NaN fails it.  Only candidates touch the volume.
//   Position  q_i = ((Rm_i0 * x + Rm_i1 * y) + Rm_i2 * z) + tm_i;  g_i = (q_i - origin_i) / voxel_size.
//   Cell      inside iff every g_i >= 0.0f && g_i < (float)(dim_i - 1), tested BEFORE any conversion to an integer: a huge or
//             NaN coordinate never becomes an index.  j_i = (int)floorf(g_i), f_i = g_i - (float)j_i; the upper corner is
//             j_i + 1.  Every index is in bounds by construction; the volume needs every dim >= 2.
//   Sample    the 8 corners c_abc (a along x); all 8 corner weights must be > weight_thresh.  F, G_0, G_1, G_2 are exactly
//             align_pair_at's expressions (tsdf_align.hip.h):
//             d_bc = c_1bc - c_0bc;  a_bc = c_0bc + f_0 * d_bc;  b_c = a_0c + f_1 * (a_1c - a_0c);  F = b_0 + f_2 * (b_1 - b_0);
//             e_c = d_0c + f_1 * (d_1c - d_0c);  G_0 = e_0 + f_2 * (e_1 - e_0);
//             h_c = a_1c - a_0c;                 G_1 = h_0 + f_2 * (h_1 - h_0);      G_2 = b_1 - b_0.
//   Pair      on the host, float32: tr = the handle's truncation distance (metres), gscale = tr / voxel_size.
//             r = F * tr (metres);  n_i = G_i * gscale (dimensionless, about unit length near a surface).
//             Rejected unless F is finite, fabsf(F) < 1.0f, fabsf(r) <= resid_thresh, every n_i is finite and
//             ((n_0 * n_0 + n_1 * n_1) + n_2 * n_2) > 0 (a NaN rejects).
//             J = (q x n, n) = (q1*n2 - q2*n1, q2*n0 - q0*n2, q0*n1 - q1*n0, n0, n1, n2): track_pair_at's order with P := q,
//             nm := n.  A step (w, tau) moves q to q + w x q + tau, so r changes by J . (w, tau).
//   Terms, system, solve, levels, status: exactly tsdf_track.hip.h's.  Per pair, in float32: J_a * J_b for a <= b (21), J_a * r
//             (6), r * r, and 1; the system is their double sum.  Cholesky with the 1e-12 * max diagonal pivot test;
//             M <- [Rodrigues(w) | tau] * M; a level ends when |w| < eps_rot and |tau| < eps_trans.  Levels n_levels-1 .. 0,
//             iters[l] iterations each.  status 2 = lost (fewer pairs than min_pairs, or a failed pivot), else 0 when the last
//             level that ran ended by the test, else 1.
//   Result    velo2world = base2world * [M; 0 0 0 1] (4 x 4, double from the float32 base2world, sums over k left to right),
//             each entry rounded to float32, last row 0 0 0 1; on a lost run it is the guess's own bits, all 16.  pairs and
//             rmse = sqrt(sum r^2 / pairs) (metres) are those of the last iteration that ran.
//
// LIMITS.  The residual exists only inside the truncation band of an observed surface, so the basin is about one truncation
// distance of displacement; the coarse levels subsample the scan, they do not widen the basin.  A scan is taken as rigid: it
// is not de-skewed for the motion during its sweep, and there are no robust weights.  The library decides nothing: whether
// the result is trusted is the caller's call from status, pairs and rmse.  The defaults (tsdf_scan_track_params_default) are
// choices, not measurements.
//
// MAPPING.  scan_track_pairs: one lane per selected point, lane index = the selected point's ordinal, walked by a fixed-order
// grid-stride loop over at most kTrackMaxBlocks 256-lane workgroups.  Each lane loads its point as one float4 (16 bytes; at
// s = 1 a wavefront reads 1 KiB in one piece, at s = 2 and 4 every second or fourth 16 bytes of 2 or 4 KiB).  The candidate
// test is made on that load alone; a wavefront with no candidate is skipped by ballot, and the 16 gathers of the volume are
// issued only under the inside test: points out of range, flagged or outside the grid cost one load and a few compares.
// Consecutive points of a spinning scanner are neighbours on one ring -- in a KITTI scan 64 consecutive points span about
// 11 degrees of azimuth on one beam, on a wall 10 m away some 2 m of one line; in firing order they are the beams of one
// firing, a vertical line -- so a wavefront's gathers (two x-neighbours in
// two rows of two slices per lane) fall into a few rows of two or three slices and meet in L1 / L2, as align_pairs' tile does
// by construction; nothing is sorted or binned for it.  The reduction is track_pairs' own: 29 double accumulators, __shfl_xor
// over 64 lanes (track_wave_sum), the four waves through LDS in wave order, one partial row per workgroup by plain stores.
// No atomics: equal inputs give equal bits.  track_init and track_solve (tsdf_track.hip.h) hold and advance the state; the
// finished / lost flags let the host queue every iteration of every level without a round trip.  The volume is read only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "tsdf_track.hip.h"

namespace tsdfk {

struct ScanTrackPairsParams {
    const float4 *pts;           // the scan, n_points x (x, y, z, intensity)
    const uint8_t *flags;        // one byte per point, or null
    const float *t, *w;          // the volume's TSDF and weight
    const TrackState *state;
    double *partials;            // gridDim.x rows of kTrackTerms
    float org[3], vs;
    float hi[3];                 // (float)(dim_i - 1)
    int dim[3];
    unsigned n_sel;              // selected points: ceil(n_points / s)
    unsigned n_lanes;            // n_sel rounded up to whole wavefronts (< 2^31: checked on the host)
    int s, level;
    int drop;                    // the flag value that drops a point (only read with flags)
    float rmin2, rmax2;
    float tr, gscale, wthr, rthr;
};

// The pair of the candidate point p (scanner coordinates), or false.
__device__ __forceinline__ bool scan_track_pair_at(const ScanTrackPairsParams &P, const float Rm[9], const float tm[3],
                                                   const float p[3], float J[6], float &r)
{
    float q[3], g[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        q[a] = ((Rm[3 * a] * p[0] + Rm[3 * a + 1] * p[1]) + Rm[3 * a + 2] * p[2]) + tm[a];
        g[a] = (q[a] - P.org[a]) / P.vs;
    }
    if (!(g[0] >= 0.0f && g[0] < P.hi[0] && g[1] >= 0.0f && g[1] < P.hi[1] && g[2] >= 0.0f && g[2] < P.hi[2])) return false;
    const int j0 = (int)floorf(g[0]), j1 = (int)floorf(g[1]), j2 = (int)floorf(g[2]);
    const float f0 = g[0] - (float)j0, f1 = g[1] - (float)j1, f2 = g[2] - (float)j2;
    const int64_t sy = P.dim[0], sz = (int64_t)P.dim[0] * P.dim[1];
    const int64_t r00 = j2 * sz + j1 * sy + j0, r10 = r00 + sy, r01 = r00 + sz, r11 = r01 + sy;
    const float *t = P.t, *w = P.w;
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
    r = F * P.tr;
    const float n[3] = {G0 * P.gscale, G1 * P.gscale, G2 * P.gscale};
    if (!(__builtin_isfinite(F) && fabsf(F) < 1.0f && fabsf(r) <= P.rthr)) return false;
    if (!(__builtin_isfinite(n[0]) && __builtin_isfinite(n[1]) && __builtin_isfinite(n[2]))) return false;
    if (!(((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2]) > 0.0f)) return false;
    J[0] = q[1] * n[2] - q[2] * n[1];
    J[1] = q[2] * n[0] - q[0] * n[2];
    J[2] = q[0] * n[1] - q[1] * n[0];
    J[3] = n[0]; J[4] = n[1]; J[5] = n[2];
    return true;
}

__global__ __launch_bounds__(256) void scan_track_pairs(ScanTrackPairsParams P)
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
    // n_lanes is a multiple of 64: the trip count is uniform over the wavefront
    for (unsigned idx = blockIdx.x * 256 + threadIdx.x; idx < P.n_lanes; idx += gridDim.x * 256) {
        bool cand = false;
        float p[3] = {0.0f, 0.0f, 0.0f};
        if (idx < P.n_sel) {
            const int64_t at = (int64_t)idx * P.s;
            const float4 v = P.pts[at];
            p[0] = v.x; p[1] = v.y; p[2] = v.z;
            const float d2 = (v.x * v.x + v.y * v.y) + v.z * v.z;
            cand = __builtin_isfinite(v.x) && __builtin_isfinite(v.y) && __builtin_isfinite(v.z) && d2 >= P.rmin2 && d2 <= P.rmax2;
            if (cand && P.flags != nullptr) cand = (int)P.flags[at] != P.drop;
        }
        if (__ballot(cand) == 0) continue;
        if (!cand) continue;
        float J[6], r;
        if (!scan_track_pair_at(P, Rm, tm, p, J, r)) continue;
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
