// tsdf_fuse.hip.h -- merging one fused volume into another by trilinear resampling (tsdf_fuse_volume): every voxel of a
// destination grid samples a source grid at its own position and folds the sample in as one weighted observation.  One
// operation serves two uses: merging a duplicate object into the member that should have had its frames, and moving an
// object's content into a grid that is placed or sized differently.
//
// THE RULE.  Every operation is float32 and is evaluated in the order written (the library builds with -ffp-contract=off and
// IEEE division, csrc/Makefile NUMFLAGS), so tests/fuse_spec.py, which restates it in float32 NumPy, matches the device bit
// for bit.  A constant changed here is changed there and in DESIGN.md ("N9") as well.
//
//   Pose     M = inverse(base2world_src) * base2world_dst, composed on the host with the library's invert / multiply (a singular
//            base2world_src gives the all-zero inverse, as everywhere else); it takes the destination's base frame to the
//            source's.  ratio = trunc_src / trunc_dst, on the host.
//   Position destination voxel (x0, x1, x2):  p_i = origin_dst_i + (float)x_i * vs_dst   (Integrate's voxel centre);
//            q_i = ((M_i0 * p_0 + M_i1 * p_1) + M_i2 * p_2) + M_i3;   g_i = (q_i - origin_src_i) / vs_src   (source grid
//            units, voxel centres at integers).
//   Sample   invalid unless every g_i is in [0, (float)(dim_src_i - 1)] (comparisons: false on NaN).
//            j_i = (int)floorf(g_i), f_i = g_i - (float)j_i, k_i = f_i > 0 ? j_i + 1 : j_i: the upper corner collapses onto
//            the lower one when the position is on the lattice, so every index is in bounds by construction (g_i = dim - 1
//            has f_i = 0) and a lattice-aligned position reads one voxel only.  The corner (a, b, c) takes j or k per axis.
//            F in ray_sample's order (tsdf_raycast.hip.h): along x, a_bc = c_0bc + f_0 * (c_1bc - c_0bc); along y,
//            b_c = a_0c + f_1 * (a_1c - a_0c); F = b_0 + f_2 * (b_1 - b_0).
//            w_s = the minimum of the 8 corner weights, by comparisons in the corner order 000, 100, 010, 110, 001, 101, 011,
//            111 (x first): w_s = w_000, then w_s = w < w_s ? w : w_s.
//            Valid iff every corner weight is > weight_thresh and F is finite.
//   Band     t = F * ratio (the sample in the destination's truncation units).  t <= -1.0f: the voxel is skipped, as
//            Integrate skips diff <= -trunc.  t = t > 1.0f ? 1.0f : t.
//   Update   (only when write) with t_d, w_d the destination's values:  w_d == 0.0f: tsdf = t, weight = w_s (a voxel no frame
//            has observed takes the sample's own bits);  otherwise w_n = w_d + w_s, tsdf = (t_d * w_d + t * w_s) / w_n,
//            weight = w_n: the running mean of Integrate with an observation of weight w_s.
//   Counts   four uint64, with t_d the destination's TSDF BEFORE the update and "a valid sample" = the sample is valid and the
//            band test did not skip the voxel:  sampled = valid samples;  both = of those, w_d > weight_thresh;  both_band =
//            of both, fabsf(t_d) < 1.0f && fabsf(t) < 1.0f;  agree_band = of both_band, fabsf(t_d - t) <= agree_tol.
//            Integer sums: they do not depend on the order of arrival.  "The same object" is the caller's decision from
//            agree_band / both_band, not the library's.
//   NaN      A valid sample is finite, so the update yields a NaN only where the destination already held a NaN, an infinity
//            or a weight that is not positive.  Which NaN an operation returns (sign, payload) is the hardware's choice and
//            differs between gfx950 and a host CPU; such a result is specified as "a NaN", every other result by its bits.
//
// DEVIATIONS.  Not a reference function: the reference never moves an object's TSDF (ref: src/Object.cpp:37-49 places the
// grid once, from the first masked frame).  Labels and colours of the destination are neither read nor written by this
// kernel; tsdf_fuse_carry.hip.h carries them, in a kernel queued ahead of this one.  The source is only read.
//
// MAPPING.  One lane per four x-adjacent destination voxels; a wavefront covers 8 such quads by 8 rows of one slice (32 x 8
// voxels: the 64 lanes' gathers fall into a few neighbouring source rows and meet in L1 / L2) and walks kFuseZRun slices,
// a 256-thread workgroup four such runs.  Where rows are 16-byte aligned (dim_x % 4 == 0) the destination moves as 16-byte
// loads and stores; otherwise (plain handles of any dim_x) every voxel is loaded and stored on its own behind its bounds
// predicate.  The source corners are plain gathers through L2; the hardware texture filter is not used, for the reason given
// in tsdf_raycast.hip.h.  No LDS, no barrier.  A wavefront none of whose lanes falls inside the source box leaves the slice
// after the position arithmetic without touching the destination; a lane loads its destination quad only when one of its
// voxels is inside, and stores it only when one was updated (the 16-byte path then stores the whole quad: its voxels that were
// not updated go back with the bits they were loaded with, and a quad belongs to one lane), so write == 0 writes nothing at
// all.  The counts are taken per wavefront with ballots and added by lane 0 with one atomicAdd on unsigned long long per
// counter that is not zero.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace tsdfk {

constexpr int kFuseZRun = 4;   // slices a wavefront walks: a quarter of the atomics of one slice per wavefront

struct FuseParams {
    float *dt, *dw;              // destination TSDF and weight
    const float *st, *sw;        // source
    float m[12];                 // the first three rows of M
    float od[3], os[3];          // origins
    float vsd, vss;              // voxel sizes
    float hi[3];                 // (float)(dim_src_i - 1)
    int sdim[3], ddim[3];
    float ratio, wthr, tol;
    int write;
    unsigned long long *counts;  // sampled, both, both_band, agree_band
};

// The source cell of a position already known to lie inside the source box: lower corner j, upper corner k, fractions f.
// tsdf_fuse_carry.hip.h gathers colours and labels from the same cell.
struct FuseCell {
    int j0, j1, j2, k0, k1, k2;
    float f0, f1, f2;
};

__device__ __forceinline__ FuseCell fuse_cell(float g0, float g1, float g2)
{
    FuseCell c;
    c.j0 = (int)floorf(g0); c.j1 = (int)floorf(g1); c.j2 = (int)floorf(g2);
    c.f0 = g0 - (float)c.j0; c.f1 = g1 - (float)c.j1; c.f2 = g2 - (float)c.j2;
    c.k0 = c.f0 > 0.0f ? c.j0 + 1 : c.j0; c.k1 = c.f1 > 0.0f ? c.j1 + 1 : c.j1; c.k2 = c.f2 > 0.0f ? c.j2 + 1 : c.j2;
    return c;
}

// F and w_s at a position already known to lie inside the source box; true = the sample is valid.
__device__ __forceinline__ bool fuse_sample(const FuseParams &P, float g0, float g1, float g2, float &F, float &ws)
{
    const FuseCell cell = fuse_cell(g0, g1, g2);
    const int j0 = cell.j0, j1 = cell.j1, j2 = cell.j2, k0 = cell.k0, k1 = cell.k1, k2 = cell.k2;
    const float f0 = cell.f0, f1 = cell.f1, f2 = cell.f2;
    const int64_t sy = P.sdim[0], sz = (int64_t)P.sdim[0] * P.sdim[1];
    const int64_t r00 = j2 * sz + j1 * sy, r10 = j2 * sz + k1 * sy, r01 = k2 * sz + j1 * sy, r11 = k2 * sz + k1 * sy;
    const float *t = P.st, *w = P.sw;
    const float c000 = t[r00 + j0], c100 = t[r00 + k0], c010 = t[r10 + j0], c110 = t[r10 + k0];
    const float c001 = t[r01 + j0], c101 = t[r01 + k0], c011 = t[r11 + j0], c111 = t[r11 + k0];
    const float w000 = w[r00 + j0], w100 = w[r00 + k0], w010 = w[r10 + j0], w110 = w[r10 + k0];
    const float w001 = w[r01 + j0], w101 = w[r01 + k0], w011 = w[r11 + j0], w111 = w[r11 + k0];
    const float thr = P.wthr;
    const bool wok = w000 > thr && w100 > thr && w010 > thr && w110 > thr && w001 > thr && w101 > thr && w011 > thr && w111 > thr;
    ws = w000;
    ws = w100 < ws ? w100 : ws;
    ws = w010 < ws ? w010 : ws;
    ws = w110 < ws ? w110 : ws;
    ws = w001 < ws ? w001 : ws;
    ws = w101 < ws ? w101 : ws;
    ws = w011 < ws ? w011 : ws;
    ws = w111 < ws ? w111 : ws;
    const float a00 = c000 + f0 * (c100 - c000);
    const float a10 = c010 + f0 * (c110 - c010);
    const float a01 = c001 + f0 * (c101 - c001);
    const float a11 = c011 + f0 * (c111 - c011);
    const float b0 = a00 + f1 * (a10 - a00);
    const float b1 = a01 + f1 * (a11 - a01);
    F = b0 + f2 * (b1 - b0);
    return wok && __builtin_isfinite(F);
}

// ALIGNED: dim_x % 4 == 0 (and the arrays' base is 16-byte aligned, as every allocation of the library is).
template <bool ALIGNED>
__global__ __launch_bounds__(256) void fuse_volume(FuseParams P)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int x0 = ((int)blockIdx.x * 8 + (lane & 7)) * 4;
    const int y = (int)blockIdx.y * 8 + (lane >> 3);
    const int zb = ((int)blockIdx.z * 4 + wave) * kFuseZRun;
    const bool row_in = x0 < P.ddim[0] && y < P.ddim[1];
    unsigned int n_sampled = 0, n_both = 0, n_band = 0, n_agree = 0;   // of the whole wavefront (ballots): uniform
    float p0[4];
#pragma unroll
    for (int v = 0; v < 4; ++v) p0[v] = P.od[0] + (float)(x0 + v) * P.vsd;
    const float p1 = P.od[1] + (float)y * P.vsd;
    for (int i = 0; i < kFuseZRun; ++i) {
        const int z = zb + i;
        if (z >= P.ddim[2]) break;   // uniform over the wavefront
        const float p2 = P.od[2] + (float)z * P.vsd;
        float g[4][3];
        bool in[4], any_in = false;
#pragma unroll
        for (int v = 0; v < 4; ++v) {
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                const float q = ((P.m[4 * a] * p0[v] + P.m[4 * a + 1] * p1) + P.m[4 * a + 2] * p2) + P.m[4 * a + 3];
                g[v][a] = (q - P.os[a]) / P.vss;
            }
            in[v] = row_in && (ALIGNED || x0 + v < P.ddim[0]) && g[v][0] >= 0.0f && g[v][0] <= P.hi[0] && g[v][1] >= 0.0f &&
                    g[v][1] <= P.hi[1] && g[v][2] >= 0.0f && g[v][2] <= P.hi[2];
            any_in = any_in || in[v];
        }
        if (__ballot(any_in) == 0) continue;   // the whole wavefront is outside the source box: the destination is not touched
        const int64_t base = ((int64_t)z * P.ddim[1] + y) * P.ddim[0] + x0;
        float td[4] = {1.0f, 1.0f, 1.0f, 1.0f}, wd[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        if (ALIGNED) {
            if (any_in) {
                const float4 t4 = *reinterpret_cast<const float4 *>(P.dt + base);
                const float4 w4 = *reinterpret_cast<const float4 *>(P.dw + base);
                td[0] = t4.x; td[1] = t4.y; td[2] = t4.z; td[3] = t4.w;
                wd[0] = w4.x; wd[1] = w4.y; wd[2] = w4.z; wd[3] = w4.w;
            }
        } else {
#pragma unroll
            for (int v = 0; v < 4; ++v)
                if (in[v]) {
                    td[v] = P.dt[base + v];
                    wd[v] = P.dw[base + v];
                }
        }
        bool upd[4], any_upd = false;
#pragma unroll
        for (int v = 0; v < 4; ++v) {
            float F = 0.0f, ws = 0.0f;
            bool valid = in[v] && fuse_sample(P, g[v][0], g[v][1], g[v][2], F, ws);
            float t = F * P.ratio;
            valid = valid && !(t <= -1.0f);
            t = t > 1.0f ? 1.0f : t;
            const bool both = valid && wd[v] > P.wthr;
            const bool band = both && fabsf(td[v]) < 1.0f && fabsf(t) < 1.0f;
            const bool agree = band && fabsf(td[v] - t) <= P.tol;
            n_sampled += (unsigned int)__popcll(__ballot(valid));
            n_both += (unsigned int)__popcll(__ballot(both));
            n_band += (unsigned int)__popcll(__ballot(band));
            n_agree += (unsigned int)__popcll(__ballot(agree));
            upd[v] = valid && P.write != 0;
            if (upd[v]) {
                if (wd[v] == 0.0f) {
                    td[v] = t;
                    wd[v] = ws;
                } else {
                    const float wn = wd[v] + ws;
                    td[v] = (td[v] * wd[v] + t * ws) / wn;
                    wd[v] = wn;
                }
            }
            any_upd = any_upd || upd[v];
        }
        if (ALIGNED) {
            if (any_upd) {
                *reinterpret_cast<float4 *>(P.dt + base) = make_float4(td[0], td[1], td[2], td[3]);
                *reinterpret_cast<float4 *>(P.dw + base) = make_float4(wd[0], wd[1], wd[2], wd[3]);
            }
        } else {
#pragma unroll
            for (int v = 0; v < 4; ++v)
                if (upd[v]) {
                    P.dt[base + v] = td[v];
                    P.dw[base + v] = wd[v];
                }
        }
    }
    if (lane == 0) {
        if (n_sampled) atomicAdd(P.counts + 0, (unsigned long long)n_sampled);
        if (n_both) atomicAdd(P.counts + 1, (unsigned long long)n_both);
        if (n_band) atomicAdd(P.counts + 2, (unsigned long long)n_band);
        if (n_agree) atomicAdd(P.counts + 3, (unsigned long long)n_agree);
    }
}

}  // namespace tsdfk
