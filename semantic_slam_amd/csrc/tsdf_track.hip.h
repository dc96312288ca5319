// tsdf_track.hip.h -- frame-to-model tracking: point-to-plane ICP of a live depth frame against the raycast of a fused volume
// (tsdf_track, tsdf_track_system).
//
// THE RULE.  Per-sample arithmetic is float32 in the order written (the library builds with -ffp-contract=off and IEEE
// division and sqrt, csrc/Makefile NUMFLAGS), so tests/track_spec.py, which restates it in float32 NumPy, makes every per-sample
// decision and every per-sample term bit for bit as the device does; sums and the solve are double.  A constant changed here
// is changed there and in DESIGN.md ("N6 -- tracking") as well.
//
//   Poses   C = compose_cam2base(cam2world) as Integrate composes it (float32).  C_ref: the pose the model is rendered at (the
//           guess for tsdf_track), C_cur: the pose being estimated.  On the host, in double from the float32 entries, with
//           C_ref's rotation R_r, translation t_r and C_cur's R_c, t_c (sums over k = 0, 1, 2 left to right):
//             M_R[i][j] = sum_k R_r[k][i] * R_c[k][j],   M_t[i] = sum_k R_r[k][i] * (t_c[k] - t_r[k])
//           i.e. M = C_ref^-1 * C_cur with the rigid inverse.  The kernels read Rm = (float)M_R, tm = (float)M_t.
//           The result: X = base2world * C_ref, then cam2world = X * M (4 x 4, double, sums over k left to right), each entry
//           rounded to float32.  tsdf_track starts from M = identity (C_cur = C_ref = the guess).
//   Sample  level l, s = 2^l: pixels (u, v) = (s*i, s*j) with u + s < W and v + s < H.  A depth d is valid iff d is finite,
//           near_m < d and d <= far_m, and, with a mask, mask[pixel] >= 128.  dcx(u) = ((float)u - cx) / fx,
//           dcy(v) = ((float)v - cy) / fy;  V(u, v) = (d * dcx(u), d * dcy(v), d).  With a = V(u+s, v) - V(u, v),
//           b = V(u, v+s) - V(u, v) (all three depths valid):  c = cross(b, a) = (b1*a2 - b2*a1, b2*a0 - b0*a2, b0*a1 - b1*a0),
//           len = sqrtf((c0*c0 + c1*c1) + c2*c2), which must be finite and > 0;  n = c / len (toward the camera).
//   Pair    p_i = ((Rm_i0*V0 + Rm_i1*V1) + Rm_i2*V2) + tm_i,  nl_i = (Rm_i0*n0 + Rm_i1*n1) + Rm_i2*n2.  Rejected unless p2 > 0.
//           pu = fx * (p0 / p2) + cx, pv = fy * (p1 / p2) + cy; rejected unless both are finite, -0.5f <= pu < (float)W - 0.5f
//           and -0.5f <= pv < (float)H - 0.5f.  ui = (int)floorf(pu + 0.5f), vi likewise; rejected unless 0 <= ui < W and
//           0 <= vi < H (never for images below 2^22 pixels a side; it makes every gather in-bounds by construction).
//           The model pixel (ui, vi) of the render at C_ref: depth t, normal nm; rejected unless t > 0 and nm != (0, 0, 0).
//           q = (t * dcx(ui), t * dcy(vi), t);  e = p - q;  rejected unless ((e0*e0 + e1*e1) + e2*e2) <= dist_thresh[l] *
//           dist_thresh[l] and ((nl0*nm0 + nl1*nm1) + nl2*nm2) >= cos_normal_thresh (a NaN rejects).
//   Terms   r = (nm0*e0 + nm1*e1) + nm2*e2;  J = (p x nm, nm) = (p1*nm2 - p2*nm1, p2*nm0 - p0*nm2, p0*nm1 - p1*nm0, nm0, nm1, nm2).
//           Per pair, in float32: J_a * J_b for a <= b (21, row-major upper triangle), J_a * r (6), r * r; and 1.  The system
//           is the double sum of these 29 terms over the pairs (the order of summation is the library's).  A step (w, tau)
//           moves p to p + w x p + tau, so r changes by J . (w, tau).
//   Solve   double: A = J^T J, b = J^T r, A xi = -b by Cholesky (A = L L^T, column by column; the pivot of column k is
//           A_kk - sum_{j<k} L_kj^2).  Lost: fewer pairs than min_inliers, or a pivot <= 1e-12 * max_k A_kk.  Otherwise
//           w = xi[0..2], tau = xi[3..5];  M <- [Rodrigues(w) | tau] * M (theta = |w|, R = I + sin(theta) [k]x +
//           (1 - cos(theta)) [k]x^2 with k = w / theta; R = I at theta = 0);  the level ends when |w| < eps_rot and
//           |tau| < eps_trans (after the step is applied).
//   Track   levels n_levels-1 .. 0, iters[l] iterations each (0 skips a level).  status: 2 lost (the result is the guess's own
//           bits), else 0 when the last level that ran ended by the test above, else 1.  inliers and rmse =
//           sqrt(sum r^2 / inliers) are those of the last iteration that ran.
//
// MAPPING.  track_pairs: one live sample per lane, a grid-stride loop over at most kTrackMaxBlocks 256-lane workgroups.  The
// live vertex and normal are recomputed from three depth loads (fewer bytes than a stored vertex / normal map); the model depth
// and normal are gathered from the full-resolution render.  The 29 sums stay in double registers, go across the wavefront by
// __shfl_xor over 64 lanes and across the four waves through LDS in wave order; each workgroup stores its partial row with
// plain stores.  No atomics: the same inputs give the same bits.  track_solve: one workgroup sums the partial rows in a fixed
// order (32-lane column groups over strided rows, then the eight groups in order), and one lane solves and updates the pose
// state in HBM (double M, float Rm / tm, per-level done flags, lost flag).  Both kernels of a finished level or a lost track
// read the flags and return at once, so the host queues the whole track without a round trip per iteration.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace tsdfk {

constexpr int kTrackTerms = 29;          // 21 of J^T J, 6 of J^T r, sum r^2, count
constexpr int kTrackMaxBlocks = 256;     // partial rows of one association pass

// The pose state in HBM, written by track_init and track_solve only.
struct TrackState {
    double M[12];            // rows of [M_R | M_t]
    float Rm[9], tm[3];      // float32 rounding of M, read by track_pairs
    int32_t lost;            // 1: the track is lost (every later kernel returns at once)
    int32_t done[3];         // 1: level l ended by the convergence test
    int32_t iters_run[3];
    int32_t inliers;         // pairs of the last iteration that ran
    double r2;               // sum r^2 of that iteration
    double sys[kTrackTerms]; // the summed system of the last iteration that ran
};

struct TrackPairsParams {
    const float *depth;          // the live frame, H*W
    const uint8_t *mask;         // H*W or null
    const float *model_depth;    // the render at C_ref, H*W
    const float *model_normal;   // H*W*3
    const TrackState *state;
    double *partials;            // gridDim.x rows of kTrackTerms
    float fx, fy, cx, cy, near_m, far_m;
    float dist2, cos_thresh;     // dist_thresh[l]^2 (float32 product), cos_normal_thresh
    int H, W, s, ni, nj, level;
};

struct TrackSolveParams {
    TrackState *state;
    const double *partials;
    int n_rows, level, min_inliers, system_only;
    double eps_rot, eps_trans;
};

__device__ __forceinline__ bool track_depth_ok(float d, const uint8_t *mask, int64_t px, float near_m, float far_m)
{
    return __builtin_isfinite(d) && near_m < d && d <= far_m && (mask == nullptr || mask[px] >= 128);
}

// The 29 terms of live sample (i, j) and its model pixel mp = vi * W + ui, or false when it makes no pair.
__device__ __forceinline__ bool track_pair_at(const TrackPairsParams &p, const float Rm[9], const float tm[3], int i, int j,
                                              float J[6], float &r, int64_t &mp)
{
    const int s = p.s, u = s * i, v = s * j;
    const int64_t px = (int64_t)v * p.W + u, px10 = px + s, px01 = px + (int64_t)s * p.W;
    const float d00 = p.depth[px], d10 = p.depth[px10], d01 = p.depth[px01];
    if (!(track_depth_ok(d00, p.mask, px, p.near_m, p.far_m) && track_depth_ok(d10, p.mask, px10, p.near_m, p.far_m) &&
          track_depth_ok(d01, p.mask, px01, p.near_m, p.far_m)))
        return false;
    const float dcx0 = ((float)u - p.cx) / p.fx, dcx1 = ((float)(u + s) - p.cx) / p.fx;
    const float dcy0 = ((float)v - p.cy) / p.fy, dcy1 = ((float)(v + s) - p.cy) / p.fy;
    const float V[3] = {d00 * dcx0, d00 * dcy0, d00};
    const float a[3] = {d10 * dcx1 - V[0], d10 * dcy0 - V[1], d10 - V[2]};
    const float b[3] = {d01 * dcx0 - V[0], d01 * dcy1 - V[1], d01 - V[2]};
    float n[3] = {b[1] * a[2] - b[2] * a[1], b[2] * a[0] - b[0] * a[2], b[0] * a[1] - b[1] * a[0]};
    const float len = sqrtf((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2]);
    if (!(__builtin_isfinite(len) && len > 0.0f)) return false;
    n[0] = n[0] / len; n[1] = n[1] / len; n[2] = n[2] / len;
    float P[3], nl[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        P[k] = ((Rm[3 * k] * V[0] + Rm[3 * k + 1] * V[1]) + Rm[3 * k + 2] * V[2]) + tm[k];
        nl[k] = (Rm[3 * k] * n[0] + Rm[3 * k + 1] * n[1]) + Rm[3 * k + 2] * n[2];
    }
    if (!(P[2] > 0.0f)) return false;
    const float pu = p.fx * (P[0] / P[2]) + p.cx, pv = p.fy * (P[1] / P[2]) + p.cy;
    if (!(__builtin_isfinite(pu) && __builtin_isfinite(pv) && pu >= -0.5f && pu < (float)p.W - 0.5f && pv >= -0.5f &&
          pv < (float)p.H - 0.5f))
        return false;
    const int ui = (int)floorf(pu + 0.5f), vi = (int)floorf(pv + 0.5f);
    if (ui < 0 || ui >= p.W || vi < 0 || vi >= p.H) return false;
    mp = (int64_t)vi * p.W + ui;
    const float t = p.model_depth[mp];
    const float nm[3] = {p.model_normal[3 * mp], p.model_normal[3 * mp + 1], p.model_normal[3 * mp + 2]};
    if (!(t > 0.0f) || (nm[0] == 0.0f && nm[1] == 0.0f && nm[2] == 0.0f)) return false;
    const float q[3] = {t * (((float)ui - p.cx) / p.fx), t * (((float)vi - p.cy) / p.fy), t};
    const float e[3] = {P[0] - q[0], P[1] - q[1], P[2] - q[2]};
    if (!(((e[0] * e[0] + e[1] * e[1]) + e[2] * e[2]) <= p.dist2)) return false;
    if (!(((nl[0] * nm[0] + nl[1] * nm[1]) + nl[2] * nm[2]) >= p.cos_thresh)) return false;
    r = (nm[0] * e[0] + nm[1] * e[1]) + nm[2] * e[2];
    J[0] = P[1] * nm[2] - P[2] * nm[1];
    J[1] = P[2] * nm[0] - P[0] * nm[2];
    J[2] = P[0] * nm[1] - P[1] * nm[0];
    J[3] = nm[0]; J[4] = nm[1]; J[5] = nm[2];
    return true;
}

__device__ __forceinline__ bool track_pair(const TrackPairsParams &p, const float Rm[9], const float tm[3], int i, int j,
                                           float J[6], float &r)
{
    int64_t mp;
    return track_pair_at(p, Rm, tm, i, j, J, r, mp);
}

__device__ __forceinline__ double track_wave_sum(double x)
{
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) x += __shfl_xor(x, m, 64);
    return x;
}

__global__ __launch_bounds__(256) void track_pairs(TrackPairsParams p)
{
    const TrackState *st = p.state;
    if (st->lost || st->done[p.level]) return;
    float Rm[9], tm[3];
#pragma unroll
    for (int k = 0; k < 9; ++k) Rm[k] = st->Rm[k];
#pragma unroll
    for (int k = 0; k < 3; ++k) tm[k] = st->tm[k];
    double acc[kTrackTerms];
#pragma unroll
    for (int k = 0; k < kTrackTerms; ++k) acc[k] = 0.0;
    const unsigned n = (unsigned)p.ni * (unsigned)p.nj;     // < 2^30: the image size is checked on the host
    for (unsigned idx = blockIdx.x * 256 + threadIdx.x; idx < n; idx += gridDim.x * 256) {
        const int j = (int)(idx / (unsigned)p.ni), i = (int)(idx - (unsigned)j * (unsigned)p.ni);
        float J[6], r;
        if (!track_pair(p, Rm, tm, i, j, J, r)) continue;
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
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < kTrackTerms; ++k) {
        const double x = track_wave_sum(acc[k]);
        if (lane == 0) lds[wave][k] = x;
    }
    __syncthreads();
    if (threadIdx.x < kTrackTerms) {
        const int k = threadIdx.x;
        p.partials[(int64_t)blockIdx.x * kTrackTerms + k] = ((lds[0][k] + lds[1][k]) + lds[2][k]) + lds[3][k];
    }
}

__global__ __launch_bounds__(64) void track_init(TrackState *state, TrackState init) { if (threadIdx.x == 0) *state = init; }

// A xi = -b by Cholesky; false when a pivot is <= 1e-12 * max diagonal.
__device__ __forceinline__ bool track_cholesky_solve(const double *sys, double xi[6])
{
    double A[6][6], L[6][6], y[6];
    int k = 0;
    for (int a = 0; a < 6; ++a)
        for (int b = a; b < 6; ++b) { A[a][b] = sys[k]; A[b][a] = sys[k]; ++k; }
    double dmax = A[0][0];
    for (int a = 1; a < 6; ++a) dmax = A[a][a] > dmax ? A[a][a] : dmax;
    for (int c = 0; c < 6; ++c) {
        double piv = A[c][c];
        for (int j = 0; j < c; ++j) piv -= L[c][j] * L[c][j];
        if (!(piv > 1e-12 * dmax)) return false;
        L[c][c] = sqrt(piv);
        for (int rr = c + 1; rr < 6; ++rr) {
            double x = A[rr][c];
            for (int j = 0; j < c; ++j) x -= L[rr][j] * L[c][j];
            L[rr][c] = x / L[c][c];
        }
    }
    for (int a = 0; a < 6; ++a) {          // L y = -b
        double x = -sys[21 + a];
        for (int j = 0; j < a; ++j) x -= L[a][j] * y[j];
        y[a] = x / L[a][a];
    }
    for (int a = 5; a >= 0; --a) {         // L^T xi = y
        double x = y[a];
        for (int j = a + 1; j < 6; ++j) x -= L[j][a] * xi[j];
        xi[a] = x / L[a][a];
    }
    return true;
}

__global__ __launch_bounds__(256) void track_solve(TrackSolveParams p)
{
    TrackState *st = p.state;
    if (st->lost || st->done[p.level]) return;
    __shared__ double grp[8][32];
    __shared__ double tot[kTrackTerms];
    const int col = threadIdx.x & 31, g = threadIdx.x >> 5;
    if (col < kTrackTerms) {
        double x = 0.0;
        for (int row = g; row < p.n_rows; row += 8) x += p.partials[(int64_t)row * kTrackTerms + col];
        grp[g][col] = x;
    }
    __syncthreads();
    if (threadIdx.x < kTrackTerms) {
        const int k = threadIdx.x;
        double x = grp[0][k];
        for (int q = 1; q < 8; ++q) x += grp[q][k];
        tot[k] = x;
        st->sys[k] = x;
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    const double count = tot[28];
    st->inliers = (int32_t)count;
    st->r2 = tot[27];
    if (p.system_only) return;
    st->iters_run[p.level] += 1;
    double xi[6];
    if (count < (double)p.min_inliers || !track_cholesky_solve(tot, xi)) {
        st->lost = 1;
        return;
    }
    const double w[3] = {xi[0], xi[1], xi[2]}, tau[3] = {xi[3], xi[4], xi[5]};
    const double th = sqrt((w[0] * w[0] + w[1] * w[1]) + w[2] * w[2]);
    const double tn = sqrt((tau[0] * tau[0] + tau[1] * tau[1]) + tau[2] * tau[2]);
    double R[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
    if (th > 0.0) {
        const double kx = w[0] / th, ky = w[1] / th, kz = w[2] / th, sn = sin(th), cs = 1.0 - cos(th);
        const double Kx[9] = {0, -kz, ky, kz, 0, -kx, -ky, kx, 0};
        for (int a = 0; a < 3; ++a)
            for (int b = 0; b < 3; ++b) {
                const double k2 = (Kx[3 * a] * Kx[b] + Kx[3 * a + 1] * Kx[3 + b]) + Kx[3 * a + 2] * Kx[6 + b];
                R[3 * a + b] = (R[3 * a + b] + sn * Kx[3 * a + b]) + cs * k2;
            }
    }
    double Mn[12];
    for (int a = 0; a < 3; ++a) {
        for (int b = 0; b < 3; ++b)
            Mn[4 * a + b] = (R[3 * a] * st->M[b] + R[3 * a + 1] * st->M[4 + b]) + R[3 * a + 2] * st->M[8 + b];
        Mn[4 * a + 3] = ((R[3 * a] * st->M[3] + R[3 * a + 1] * st->M[7]) + R[3 * a + 2] * st->M[11]) + tau[a];
    }
    for (int a = 0; a < 3; ++a) {
        for (int b = 0; b < 4; ++b) st->M[4 * a + b] = Mn[4 * a + b];
        for (int b = 0; b < 3; ++b) st->Rm[3 * a + b] = (float)Mn[4 * a + b];
        st->tm[a] = (float)Mn[4 * a + 3];
    }
    if (th < p.eps_rot && tn < p.eps_trans) st->done[p.level] = 1;
}

}  // namespace tsdfk
