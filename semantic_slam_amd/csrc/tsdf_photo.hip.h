// tsdf_photo.hip.h -- photometric tracking: an intensity residual of a live RGB-D frame against the colour fused into the volume,
// solved together with the point-to-plane system of tsdf_track.hip.h (tsdf_track_rgbd, tsdf_track_rgbd_system,
// tsdf_render_intensity).
//
// THE RULE.  Per-sample arithmetic is float32 in the order written (the library builds with -ffp-contract=off and IEEE
// division and sqrt, csrc/Makefile NUMFLAGS), so tests/photo_spec.py, which restates it in float32 NumPy, makes every per-sample
// decision and every per-sample term bit for bit as the device does; sums and the solve are double.  A constant changed here
// is changed there and in DESIGN.md ("N13 -- photometric tracking") as well.  Poses, Sample's depth test, Solve and Track are
// those of tsdf_track.hip.h; only what differs is stated.
//
//   Luminance  Y(r, g, b) = ((0.299f * (float)r + 0.587f * (float)g) + 0.114f * (float)b) / 255.0f from 8-bit channels: the
//              live rgb bytes (channel 0 = R) and a voxel's packed 0x00BBGGRR alike.  Valid intensities lie in [0, 1]; an
//              invalid one is stored as -1.0f and tested as !(I >= 0.0f).
//   Model      level 0, one value per pixel (u, v) of the depth render t at C_ref.  t > 0: dcx, dcy, gd_i, go_i as the raycast
//              rule's Ray (ray_setup with the same arguments: the same bits), g*_i = go_i + t * gd_i, and the raycast rule's
//              Sample at g*: valid iff every g*_i is in [0, hi_i] and all 8 corner weights are > weight_thresh; the cell j_i
//              and fractions f_i are Sample's.  With y_xyz = Y of the colour at j + (x, y, z):
//              a_yz = y_0yz + f_0 * (y_1yz - y_0yz) for yz = 00, 10, 01, 11;  b_z = a_0z + f_1 * (a_1z - a_0z);
//              I = b_0 + f_2 * (b_1 - b_0).  t <= 0 or an invalid Sample: -1.
//   Pyramid    level l+1 from level l, sizes W_{l+1} = W_l / 2, H_{l+1} = H_l / 2 (integer division):
//              I(i, j) = ((I00 + I10) + (I01 + I11)) * 0.25f over the children (2i + x, 2j + y), valid iff all four are.
//              The live pyramid starts from Y of the rgb bytes (every pixel valid), the model's from Model.
//   Pair       level l, s = 2^l, h = (float)(s - 1) * 0.5f (0, 0.5f, 1.5f).  Samples (i, j) and (u, v) = (s*i, s*j) as
//              tsdf_track.hip.h's Sample (u + s < W, v + s < H); d = depth[v][u] must pass its depth test (that pixel's mask byte).
//              V = (d * dcx, d * dcy, d) with dcx = (((float)u + h) - cx) / fx, dcy = (((float)v + h) - cy) / fy.
//              p_i = ((Rm_i0*V0 + Rm_i1*V1) + Rm_i2*V2) + tm_i; rejected unless p2 > 0; pu, pv, their bounds and (ui, vi) exactly
//              as tsdf_track.hip.h's Pair.  x = (pu - h) / (float)s, y = (pv - h) / (float)s; x0 = floorf(x), y0 = floorf(y);
//              rejected unless x0 >= 0, x0 + 1 <= (float)(W_l - 1), y0 >= 0, y0 + 1 <= (float)(H_l - 1) (a level with W_l < 2 or
//              H_l < 2 has no footprint).  I00, I10, I01, I11: the model level at (x0, y0), (x0+1, y0), (x0, y0+1), (x0+1, y0+1),
//              all four valid, and the live level's L = I_live_l(i, j) valid.
//   Occlusion  t = model depth at full-resolution pixel (ui, vi); rejected unless t > 0 and fabsf(p2 - t) <= dist_thresh[l].
//   Residual   ax = x - x0, ay = y - y0;  top = I00 + ax * (I10 - I00), bot = I01 + ax * (I11 - I01), Im = top + ay * (bot - top);
//              r = Im - L; rejected unless fabsf(r) <= intensity_thresh (a NaN rejects).
//   Gradient   gx = (1 - ay) * (I10 - I00) + ay * (I11 - I01),  gy = (1 - ax) * (I01 - I00) + ax * (I11 - I10) (the exact
//              derivative of the interpolant, per level pixel);  a = (fx * gx) / (float)s,  b = (fy * gy) / (float)s.
//   Terms      Jp = (a / p2, b / p2, -(((a*p0 + b*p1) / p2) / p2));
//              J = (p x Jp, Jp) = (p1*Jp2 - p2*Jp1, p2*Jp0 - p0*Jp2, p0*Jp1 - p1*Jp0, Jp0, Jp1, Jp2): a step (w, tau) moves p to
//              p + w x p + tau, so r changes by J . (w, tau).  Per pair the 29 float32 terms of tsdf_track.hip.h's Terms, summed
//              in double.
//   Solve      both blocks of partial rows are summed as track_solve sums one; with lam2 = (double)photo_weight *
//              (double)photo_weight, entry k < 27 of the combined system is g_k + lam2 * p_k.  Lost: fewer GEOMETRIC pairs
//              than min_inliers, or a failed pivot of the combined A.  The step, the state and the convergence test are
//              track_solve's.  TrackState holds the geometric count, sum r^2 and system as after track_solve; PhotoState holds
//              the photometric ones.
//
// MAPPING.  photo_luma, photo_model_intensity, photo_halve: one output pixel per lane, 256-lane workgroups over the flat
// index.  photo_pairs: as track_pairs -- one sample per lane, a grid-stride loop over at most kTrackMaxBlocks workgroups of
// 256, the 29 sums in double registers, across the wavefront by __shfl_xor, across the four waves through LDS in wave order,
// one partial row per workgroup with plain stores, no atomics.  It is a kernel of its own beside track_pairs: 29 double sums
// are 58 VGPRs in each, and track_pairs keeps its bits.  photo_solve: one workgroup, track_solve's reduction once per block.
// Every gather is in-bounds by construction: the model Sample loads only after g* has been checked to lie in [0, hi] (so
// j_i + 1 <= dim_i - 1); a halve reads children 2i + 1 <= 2 * (W_l / 2) - 1 <= W_l - 1; the live sample has u + s < W, so
// i < W / s = W_l; the footprint is checked as floats against [0, W_l - 1] x [0, H_l - 1] before it becomes an index; (ui, vi)
// is checked against the image as in track_pair_at.
#pragma once
#include "tsdf_raycast.hip.h"
#include "tsdf_track.hip.h"

namespace tsdfk {

constexpr int kPhotoLevels = 3;

// The photometric side of the state, written by photo_init and photo_solve only.
struct PhotoState {
    int32_t pairs;           // photometric pairs of the last iteration that ran
    int32_t pad;
    double r2;               // sum r^2 of that iteration
    double sys[kTrackTerms]; // the summed photometric system of that iteration (unweighted)
};

struct PhotoModelParams {
    RayVolume vol;
    const uint32_t *colour;  // fused colours, packed 0x00BBGGRR
    const float *depth;      // the render at C_ref, H*W
    float *out;              // level 0 of the model pyramid, H*W
    float fx, fy, cx, cy, near_m, far_m, wthr;
    int H, W;
};

struct PhotoPairsParams {
    const float *depth;          // the live frame, H*W
    const uint8_t *mask;         // H*W or null
    const float *live;           // level l of the live pyramid, Hl*Wl
    const float *model;          // level l of the model pyramid, Hl*Wl
    const float *model_depth;    // the render at C_ref, H*W
    const TrackState *state;
    double *partials;            // gridDim.x rows of kTrackTerms
    float fx, fy, cx, cy, near_m, far_m;
    float dist, ithr;            // dist_thresh[l], intensity_thresh
    int H, W, Hl, Wl, s, ni, nj, level;
};

struct PhotoSolveParams {
    TrackState *state;
    PhotoState *photo;
    const double *geo_partials, *photo_partials;
    int geo_rows, photo_rows, level, min_inliers, system_only;
    double lam2, eps_rot, eps_trans;
};

__device__ __forceinline__ float photo_luma_of(uint32_t r, uint32_t g, uint32_t b)
{
    return ((0.299f * (float)r + 0.587f * (float)g) + 0.114f * (float)b) / 255.0f;
}

__device__ __forceinline__ float photo_luma_packed(uint32_t c) { return photo_luma_of(c & 255u, (c >> 8) & 255u, (c >> 16) & 255u); }

// Level 0 of the live pyramid from the rgb bytes.
__global__ __launch_bounds__(256) void photo_luma(const uint8_t *rgb, float *out, int n)
{
    const int px = blockIdx.x * 256 + threadIdx.x;      // n <= 2^30: the image size is checked on the host
    if (px >= n) return;
    const uint8_t *c = rgb + (size_t)px * 3u;
    out[px] = photo_luma_of(c[0], c[1], c[2]);
}

__global__ __launch_bounds__(256) void photo_model_intensity(PhotoModelParams p)
{
    const int px = blockIdx.x * 256 + threadIdx.x;
    if (px >= p.H * p.W) return;
    const int v = px / p.W, u = px - v * p.W;
    const RayVolume &V = p.vol;
    const float t = p.depth[px];
    float I = -1.0f;
    if (t > 0.0f) {
        const float dcx = ((float)u - p.cx) / p.fx, dcy = ((float)v - p.cy) / p.fy;
        float gd[3], t_enter, t_exit;
        ray_setup(V, dcx, dcy, p.near_m, p.far_m, gd, t_enter, t_exit);      // the same gd bits as in the march
        const float g0 = V.go[0] + t * gd[0], g1 = V.go[1] + t * gd[1], g2 = V.go[2] + t * gd[2];
        if (g0 >= 0.0f && g0 <= V.hi[0] && g1 >= 0.0f && g1 <= V.hi[1] && g2 >= 0.0f && g2 <= V.hi[2]) {
            const int j0 = min((int)floorf(g0), V.dim[0] - 2);
            const int j1 = min((int)floorf(g1), V.dim[1] - 2);
            const int j2 = min((int)floorf(g2), V.dim[2] - 2);
            const float f0 = g0 - (float)j0, f1 = g1 - (float)j1, f2 = g2 - (float)j2;
            const int64_t sy = V.dim[0], sz = (int64_t)V.dim[0] * V.dim[1];
            const int64_t b = (int64_t)j2 * sz + (int64_t)j1 * sy + j0;
            const float *w = V.weight + b;
            const uint32_t *c = p.colour + b;
            const float wthr = p.wthr;
            const bool wok = w[0] > wthr && w[1] > wthr && w[sy] > wthr && w[sy + 1] > wthr &&
                             w[sz] > wthr && w[sz + 1] > wthr && w[sz + sy] > wthr && w[sz + sy + 1] > wthr;
            if (wok) {
                const float c000 = photo_luma_packed(c[0]), c100 = photo_luma_packed(c[1]);
                const float c010 = photo_luma_packed(c[sy]), c110 = photo_luma_packed(c[sy + 1]);
                const float c001 = photo_luma_packed(c[sz]), c101 = photo_luma_packed(c[sz + 1]);
                const float c011 = photo_luma_packed(c[sz + sy]), c111 = photo_luma_packed(c[sz + sy + 1]);
                const float a00 = c000 + f0 * (c100 - c000);
                const float a10 = c010 + f0 * (c110 - c010);
                const float a01 = c001 + f0 * (c101 - c001);
                const float a11 = c011 + f0 * (c111 - c011);
                const float b0 = a00 + f1 * (a10 - a00);
                const float b1 = a01 + f1 * (a11 - a01);
                I = b0 + f2 * (b1 - b0);
            }
        }
    }
    p.out[px] = I;
}

// Level l+1 (Wo x Ho) from level l (row length Wi).
__global__ __launch_bounds__(256) void photo_halve(const float *in, float *out, int Wi, int Wo, int Ho)
{
    const int px = blockIdx.x * 256 + threadIdx.x;
    if (px >= Wo * Ho) return;
    const int j = px / Wo, i = px - j * Wo;
    const float *c = in + (int64_t)(2 * j) * Wi + 2 * i;
    const float I00 = c[0], I10 = c[1], I01 = c[Wi], I11 = c[Wi + 1];
    const bool ok = I00 >= 0.0f && I10 >= 0.0f && I01 >= 0.0f && I11 >= 0.0f;
    out[px] = ok ? ((I00 + I10) + (I01 + I11)) * 0.25f : -1.0f;
}

// J and r of live sample (i, j), or false when it makes no pair.
__device__ __forceinline__ bool photo_pair(const PhotoPairsParams &p, const float Rm[9], const float tm[3], int i, int j,
                                           float J[6], float &r)
{
    const int s = p.s, u = s * i, v = s * j;
    const int64_t px = (int64_t)v * p.W + u;
    const float d = p.depth[px];
    if (!track_depth_ok(d, p.mask, px, p.near_m, p.far_m)) return false;
    const float h = (float)(s - 1) * 0.5f, fs = (float)s;
    const float dcx = (((float)u + h) - p.cx) / p.fx, dcy = (((float)v + h) - p.cy) / p.fy;
    const float V[3] = {d * dcx, d * dcy, d};
    float P[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) P[k] = ((Rm[3 * k] * V[0] + Rm[3 * k + 1] * V[1]) + Rm[3 * k + 2] * V[2]) + tm[k];
    if (!(P[2] > 0.0f)) return false;
    const float pu = p.fx * (P[0] / P[2]) + p.cx, pv = p.fy * (P[1] / P[2]) + p.cy;
    if (!(__builtin_isfinite(pu) && __builtin_isfinite(pv) && pu >= -0.5f && pu < (float)p.W - 0.5f && pv >= -0.5f &&
          pv < (float)p.H - 0.5f))
        return false;
    const int ui = (int)floorf(pu + 0.5f), vi = (int)floorf(pv + 0.5f);
    if (ui < 0 || ui >= p.W || vi < 0 || vi >= p.H) return false;
    const float x = (pu - h) / fs, y = (pv - h) / fs;
    const float x0 = floorf(x), y0 = floorf(y);
    if (!(x0 >= 0.0f && x0 + 1.0f <= (float)(p.Wl - 1) && y0 >= 0.0f && y0 + 1.0f <= (float)(p.Hl - 1))) return false;
    const float *m = p.model + (int64_t)(int)y0 * p.Wl + (int)x0;
    const float I00 = m[0], I10 = m[1], I01 = m[p.Wl], I11 = m[p.Wl + 1];
    const float L = p.live[(int64_t)j * p.Wl + i];
    if (!(I00 >= 0.0f && I10 >= 0.0f && I01 >= 0.0f && I11 >= 0.0f && L >= 0.0f)) return false;
    const float t = p.model_depth[(int64_t)vi * p.W + ui];
    if (!(t > 0.0f) || !(fabsf(P[2] - t) <= p.dist)) return false;
    const float ax = x - x0, ay = y - y0;
    const float top = I00 + ax * (I10 - I00), bot = I01 + ax * (I11 - I01);
    const float Im = top + ay * (bot - top);
    r = Im - L;
    if (!(fabsf(r) <= p.ithr)) return false;
    const float gx = (1.0f - ay) * (I10 - I00) + ay * (I11 - I01);
    const float gy = (1.0f - ax) * (I01 - I00) + ax * (I11 - I10);
    const float a = (p.fx * gx) / fs, b = (p.fy * gy) / fs;
    const float Jp[3] = {a / P[2], b / P[2], -(((a * P[0] + b * P[1]) / P[2]) / P[2])};
    J[0] = P[1] * Jp[2] - P[2] * Jp[1];
    J[1] = P[2] * Jp[0] - P[0] * Jp[2];
    J[2] = P[0] * Jp[1] - P[1] * Jp[0];
    J[3] = Jp[0]; J[4] = Jp[1]; J[5] = Jp[2];
    return true;
}

__global__ __launch_bounds__(256) void photo_pairs(PhotoPairsParams p)
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
        if (!photo_pair(p, Rm, tm, i, j, J, r)) continue;
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

__global__ __launch_bounds__(64) void photo_init(PhotoState *state)
{
    if (threadIdx.x == 0) *state = PhotoState{};
}

// track_solve's sum of one block of partial rows into tot (every lane of the workgroup calls it).
__device__ __forceinline__ void photo_sum_rows(const double *partials, int n_rows, double (*grp)[32], double *tot)
{
    const int col = threadIdx.x & 31, g = threadIdx.x >> 5;
    if (col < kTrackTerms) {
        double x = 0.0;
        for (int row = g; row < n_rows; row += 8) x += partials[(int64_t)row * kTrackTerms + col];
        grp[g][col] = x;
    }
    __syncthreads();
    if (threadIdx.x < kTrackTerms) {
        const int k = threadIdx.x;
        double x = grp[0][k];
        for (int q = 1; q < 8; ++q) x += grp[q][k];
        tot[k] = x;
    }
    __syncthreads();
}

__global__ __launch_bounds__(256) void photo_solve(PhotoSolveParams p)
{
    TrackState *st = p.state;
    if (st->lost || st->done[p.level]) return;
    __shared__ double grp[8][32];
    __shared__ double tot_g[kTrackTerms], tot_p[kTrackTerms];
    photo_sum_rows(p.geo_partials, p.geo_rows, grp, tot_g);
    photo_sum_rows(p.photo_partials, p.photo_rows, grp, tot_p);
    if (threadIdx.x < kTrackTerms) {
        st->sys[threadIdx.x] = tot_g[threadIdx.x];
        p.photo->sys[threadIdx.x] = tot_p[threadIdx.x];
    }
    if (threadIdx.x != 0) return;
    const double count = tot_g[28];
    st->inliers = (int32_t)count;
    st->r2 = tot_g[27];
    p.photo->pairs = (int32_t)tot_p[28];
    p.photo->r2 = tot_p[27];
    if (p.system_only) return;
    st->iters_run[p.level] += 1;
    double sys[kTrackTerms], xi[6];
    for (int k = 0; k < 27; ++k) sys[k] = tot_g[k] + p.lam2 * tot_p[k];
    sys[27] = tot_g[27];
    sys[28] = tot_g[28];
    if (count < (double)p.min_inliers || !track_cholesky_solve(sys, xi)) {
        st->lost = 1;
        return;
    }
    // the step and the test of track_solve
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
