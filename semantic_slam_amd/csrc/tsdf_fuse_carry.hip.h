// tsdf_fuse_carry.hip.h -- carrying colour and labels through a merge (tsdf_fuse_volume_carry): the destination voxels a merge
// updates also take the source's colour, folded in with the weights the merge folds the TSDF in with, and the source's label
// evidence, folded in as one observation.  A re-gridded object keeps its colour and its instance votes; a merged duplicate
// adds its votes to its twin's.
//
// THE RULE.  float32, evaluated in the order written, as tsdf_fuse.hip.h's; tests/fuse_carry_spec.py restates it bit for bit.
//
//   Shared   The positions g, the cell (j, f, k: fuse_cell), the corner order, w_s, validity and the band skip are
//            tsdf_fuse.hip.h's, through the same functions.  A destination voxel is CARRIED iff the merge updates it: a valid
//            sample that the band test did not skip, so the carried voxels number counts->sampled.  w_d is the destination's
//            weight BEFORE the merge and w_n = w_d + w_s: the kernel of this file runs ahead of fuse_volume on the same stream.
//   Colour   (packed 0x00BBGGRR, tsdf_colour.hip.h) per channel, shift s = 0, 8, 16: each corner's channel is
//            (float)((col >> s) & 255); c_s is the eight values interpolated along x, then y, then z with the cell's f and F's
//            expression shape (a = c0 + f * (c1 - c0)).  x = c_s when w_d == 0.0f, otherwise
//            x = ((float)c_d * w_d + c_s * w_s) / w_n; r = roundf(x);
//            channel = r >= 255.0f ? 255 : (r >= 0.0f ? (uint32_t)r : 0): both comparisons are false on a NaN, which gives 0,
//            and no value outside [0, 255) is ever converted.  The top byte is 0.  On the lattice (f == 0) a voxel no frame
//            has observed takes the source colour's bits.  This is integrate_colour's running mean (w_old = w_new - 1 there)
//            with an observation of weight w_s.  Only a writing call (write == 1) touches colour; colour has no counts.
//   Labels   The source voxel is the nearest corner of the cell: n_i = f_i >= 0.5f ? k_i : j_i (in bounds as k is).  With
//            (L_s, Fp_s, Bp_s) read there, L_s == 0 leaves the destination voxel alone; otherwise, with the destination's
//            prob_thd (tsdf_labels_enable):
//              adopted   L_d == 0:      the voxel takes the three source values' bits;
//              agreed    L_d == L_s:    Fp_d = Fp_d + Fp_s, Bp_d = Bp_d + Bp_s;
//              opposed   otherwise:     Bp_d = Bp_d + Fp_s; then, if Fp_d / (Fp_d + Bp_d) < prob_thd, the voxel takes the three
//                                       source values' bits (flipped, a subset of opposed).
//            integrate_labels' rule (tsdf_labels.hip.h) with the source voxel as one observation of label L_s and score
//            Fp_s: a source voxel holding one frame's vote (L, s, 0) is folded in exactly as that frame would have been.
//   Counts   four uint64 over the carried voxels with L_s != 0: adopted, agreed, opposed, flipped.  Integer sums, taken
//            whether or not write is set.
//   NaN      Fp / Bp are specified by their bits, a NaN as "a NaN" (tsdf_fuse.hip.h).
//
// DEVIATIONS.  Not a reference function.  A trilinear or majority vote over the cell's labels, counts of colour agreement,
// z-slab and tsdf_group handles are out of scope.
//
// MAPPING.  fuse_volume's: one lane per x-quad of the destination (handles with colour or labels have dim_x % 4 == 0, so only
// the 16-byte path exists), a wavefront covers 8 quads by 8 rows and walks kFuseZRun slices; no LDS, no barrier.  A wavefront
// wholly outside the source box leaves the slice after the position arithmetic.  A lane first samples its four voxels
// (fuse_sample: 16 gathers each), loads its destination quads (16 bytes of weight, colour, Fp, Bp; 8 bytes of labels) only
// when one of its voxels is carried -- the label quads only when a carried voxel's source label is not 0 -- and stores a quad
// only when one of its voxels was updated, so write == 0 writes nothing.  The label counts are taken with ballots and added
// by lane 0 with one atomicAdd per counter that is not zero.
#pragma once
#include "tsdf_fuse.hip.h"

namespace tsdfk {

struct FuseCarryParams {
    FuseParams g;                  // the merge's own block: dw is read (the weights before the merge), dt and counts are not used
    uint32_t *dcol;                // destination attributes (those of a template argument that is false are not touched)
    uint16_t *dlab;
    float *dfp, *dbp;
    const uint32_t *scol;          // source attributes
    const uint16_t *slab;
    const float *sfp, *sbp;
    float prob_thd;                // the destination's
    unsigned long long *counts;    // adopted, agreed, opposed, flipped
};

// One channel of the eight corner colours (corner order 000, 100, 010, 110, 001, 101, 011, 111), interpolated as F is.
__device__ __forceinline__ float carry_channel(const uint32_t c[8], int s, float f0, float f1, float f2)
{
    const float c000 = (float)((c[0] >> s) & 255u), c100 = (float)((c[1] >> s) & 255u);
    const float c010 = (float)((c[2] >> s) & 255u), c110 = (float)((c[3] >> s) & 255u);
    const float c001 = (float)((c[4] >> s) & 255u), c101 = (float)((c[5] >> s) & 255u);
    const float c011 = (float)((c[6] >> s) & 255u), c111 = (float)((c[7] >> s) & 255u);
    const float a00 = c000 + f0 * (c100 - c000);
    const float a10 = c010 + f0 * (c110 - c010);
    const float a01 = c001 + f0 * (c101 - c001);
    const float a11 = c011 + f0 * (c111 - c011);
    const float b0 = a00 + f1 * (a10 - a00);
    const float b1 = a01 + f1 * (a11 - a01);
    return b0 + f2 * (b1 - b0);
}

__device__ __forceinline__ uint32_t carry_blend(uint32_t cd, float cs, float wd, float ws)
{
    float x = cs;
    if (!(wd == 0.0f)) {
        const float wn = wd + ws;
        x = ((float)cd * wd + cs * ws) / wn;
    }
    const float r = roundf(x);
    return r >= 255.0f ? 255u : (r >= 0.0f ? (uint32_t)r : 0u);
}

template <bool COLOUR, bool LABELS>
__global__ __launch_bounds__(256) void fuse_carry(FuseCarryParams C)
{
    const FuseParams &P = C.g;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int x0 = ((int)blockIdx.x * 8 + (lane & 7)) * 4;
    const int y = (int)blockIdx.y * 8 + (lane >> 3);
    const int zb = ((int)blockIdx.z * 4 + wave) * kFuseZRun;
    const bool row_in = x0 < P.ddim[0] && y < P.ddim[1];
    const bool write = P.write != 0;
    const int64_t sy = P.sdim[0], sz = (int64_t)P.sdim[0] * P.sdim[1];
    unsigned int n_adopted = 0, n_agreed = 0, n_opposed = 0, n_flipped = 0;   // of the whole wavefront (ballots): uniform
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
            in[v] = row_in && g[v][0] >= 0.0f && g[v][0] <= P.hi[0] && g[v][1] >= 0.0f && g[v][1] <= P.hi[1] &&
                    g[v][2] >= 0.0f && g[v][2] <= P.hi[2];
            any_in = any_in || in[v];
        }
        if (__ballot(any_in) == 0) continue;   // the whole wavefront is outside the source box: nothing is touched
        // the carried set: the voxels fuse_volume will update
        bool car[4], any_car = false;
        float ws[4];
#pragma unroll
        for (int v = 0; v < 4; ++v) {
            float F = 0.0f;
            ws[v] = 0.0f;
            const bool valid = in[v] && fuse_sample(P, g[v][0], g[v][1], g[v][2], F, ws[v]);
            const float t = F * P.ratio;
            car[v] = valid && !(t <= -1.0f);
            any_car = any_car || car[v];
        }
        if (__ballot(any_car) == 0) continue;
        const int64_t base = ((int64_t)z * P.ddim[1] + y) * P.ddim[0] + x0;
        if (COLOUR && any_car) {
            const float4 w4 = *reinterpret_cast<const float4 *>(P.dw + base);
            const uint4 c4 = *reinterpret_cast<const uint4 *>(C.dcol + base);
            const float wd[4] = {w4.x, w4.y, w4.z, w4.w};
            uint32_t col[4] = {c4.x, c4.y, c4.z, c4.w};
#pragma unroll
            for (int v = 0; v < 4; ++v) {
                if (!car[v]) continue;
                const FuseCell k = fuse_cell(g[v][0], g[v][1], g[v][2]);
                const int64_t r00 = k.j2 * sz + k.j1 * sy, r10 = k.j2 * sz + k.k1 * sy;
                const int64_t r01 = k.k2 * sz + k.j1 * sy, r11 = k.k2 * sz + k.k1 * sy;
                const uint32_t *s = C.scol;
                const uint32_t c[8] = {s[r00 + k.j0], s[r00 + k.k0], s[r10 + k.j0], s[r10 + k.k0],
                                       s[r01 + k.j0], s[r01 + k.k0], s[r11 + k.j0], s[r11 + k.k0]};
                const uint32_t r = carry_blend(col[v] & 255u, carry_channel(c, 0, k.f0, k.f1, k.f2), wd[v], ws[v]);
                const uint32_t gr = carry_blend((col[v] >> 8) & 255u, carry_channel(c, 8, k.f0, k.f1, k.f2), wd[v], ws[v]);
                const uint32_t b = carry_blend((col[v] >> 16) & 255u, carry_channel(c, 16, k.f0, k.f1, k.f2), wd[v], ws[v]);
                col[v] = (b << 16) | (gr << 8) | r;
            }
            if (write) *reinterpret_cast<uint4 *>(C.dcol + base) = make_uint4(col[0], col[1], col[2], col[3]);
        }
        if (LABELS) {
            int64_t at[4];
            uint16_t Ls[4];
            bool hit = false;
#pragma unroll
            for (int v = 0; v < 4; ++v) {
                Ls[v] = 0;
                at[v] = 0;
                if (car[v]) {
                    const FuseCell k = fuse_cell(g[v][0], g[v][1], g[v][2]);
                    const int n0 = k.f0 >= 0.5f ? k.k0 : k.j0, n1 = k.f1 >= 0.5f ? k.k1 : k.j1, n2 = k.f2 >= 0.5f ? k.k2 : k.j2;
                    at[v] = n2 * sz + n1 * sy + n0;
                    Ls[v] = C.slab[at[v]];
                }
                hit = hit || Ls[v] != 0;
            }
            bool adopted[4] = {false, false, false, false}, agreed[4] = {false, false, false, false};
            bool opposed[4] = {false, false, false, false}, flipped[4] = {false, false, false, false};
            if (hit) {
                const ushort4 L4 = *reinterpret_cast<const ushort4 *>(C.dlab + base);
                const float4 F4 = *reinterpret_cast<const float4 *>(C.dfp + base);
                const float4 B4 = *reinterpret_cast<const float4 *>(C.dbp + base);
                uint16_t L[4] = {L4.x, L4.y, L4.z, L4.w};
                float Fv[4] = {F4.x, F4.y, F4.z, F4.w}, Bv[4] = {B4.x, B4.y, B4.z, B4.w};
#pragma unroll
                for (int v = 0; v < 4; ++v) {
                    if (Ls[v] == 0) continue;
                    const float Fs = C.sfp[at[v]], Bs = C.sbp[at[v]];
                    if (L[v] == 0) {
                        adopted[v] = true;
                        L[v] = Ls[v]; Fv[v] = Fs; Bv[v] = Bs;
                    } else if (L[v] == Ls[v]) {
                        agreed[v] = true;
                        Fv[v] = Fv[v] + Fs; Bv[v] = Bv[v] + Bs;
                    } else {
                        opposed[v] = true;
                        Bv[v] = Bv[v] + Fs;
                        if (Fv[v] / (Fv[v] + Bv[v]) < C.prob_thd) {
                            flipped[v] = true;
                            L[v] = Ls[v]; Fv[v] = Fs; Bv[v] = Bs;
                        }
                    }
                }
                if (write) {
                    ushort4 Lo; Lo.x = L[0]; Lo.y = L[1]; Lo.z = L[2]; Lo.w = L[3];
                    *reinterpret_cast<ushort4 *>(C.dlab + base) = Lo;
                    *reinterpret_cast<float4 *>(C.dfp + base) = make_float4(Fv[0], Fv[1], Fv[2], Fv[3]);
                    *reinterpret_cast<float4 *>(C.dbp + base) = make_float4(Bv[0], Bv[1], Bv[2], Bv[3]);
                }
            }
#pragma unroll
            for (int v = 0; v < 4; ++v) {
                n_adopted += (unsigned int)__popcll(__ballot(adopted[v]));
                n_agreed += (unsigned int)__popcll(__ballot(agreed[v]));
                n_opposed += (unsigned int)__popcll(__ballot(opposed[v]));
                n_flipped += (unsigned int)__popcll(__ballot(flipped[v]));
            }
        }
    }
    if (LABELS && lane == 0) {
        if (n_adopted) atomicAdd(C.counts + 0, (unsigned long long)n_adopted);
        if (n_agreed) atomicAdd(C.counts + 1, (unsigned long long)n_agreed);
        if (n_opposed) atomicAdd(C.counts + 2, (unsigned long long)n_opposed);
        if (n_flipped) atomicAdd(C.counts + 3, (unsigned long long)n_flipped);
    }
}

}  // namespace tsdfk
