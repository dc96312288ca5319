// tsdf_associate.hip.h -- which fused object each instance mask of a live frame shows: the counting kernel of tsdf_associate_count /
// tsdf_batch_associate (the host assignment is in tsdf_capi.hip).
//
// THE RULE.  Per-pixel tests are float32 in the order written (the library builds with -ffp-contract=off, csrc/Makefile
// NUMFLAGS), so tests/associate_spec.py, which restates them in NumPy, gives the same counts word for word.  A change here is a
// change there and in include/tsdf_hip.h and DESIGN.md ("N7 -- association") as well.
//
//   Inputs  a render (member[p], rdepth[p]) -- raycast_batch's, or the caller's for tsdf_associate_count; the live depth d = depth[p];
//           K instance masks, mask k of pixel p at masks[k * H * W + p]; M members.  p = v * W + u runs over the H * W pixels.
//   Live    valid iff isfinite(d) && near_m < d && d <= far_m (track_depth_ok without a mask).
//   Mask    pixel p is in mask k iff masks[k * H * W + p] >= 128.
//   Render  rendered iff 0 <= member[p] < M (raycast_batch writes -1 or a member index; any other value counts as not rendered).
//   Class   of a rendered pixel, m = member[p]:  live not valid -> 3;  else r = d - rdepth[p],  fabsf(r) <= tol -> 0 (agree),
//           r < -tol -> 1 (front: something occludes the model), otherwise 2 (behind: the camera sees through the model's
//           surface; also where rdepth is NaN).
//   Counts  uint32, one block of 3KM + 3K + 4M words:
//             overlap[k][m][c] (c < 3) at (k * M + m) * 3 + c         pixels in mask k, rendered as m, of class c
//             mask[k][j]       at 3KM + 3k + j                         j = 0: in mask k; 1: and live valid; 2: and not rendered
//             member[m][c]     at 3KM + 3K + 4m + c                    pixels rendered as m, of class c (whole image)
//           Every count is a sum of ones, so the block does not depend on the order the pixels are visited in.
//
// MAPPING.  One lane takes 4 adjacent pixels p = 4q .. 4q + 3 of the flattened image (rows are contiguous, so a quad may span
// a row end; the counts do not see rows), a 256-lane workgroup walks quads with a grid stride.  When H * W is a multiple of 4
// and every pointer is aligned (VEC), the member, render and live loads are 16-byte loads and each mask is one 4-byte load per
// lane; otherwise each of the 4 pixels is loaded alone behind p < H * W.  No load is issued for a pixel at or past H * W, and a
// member index only addresses LDS after 0 <= m - m0 < MT has been tested.
// Counts go to LDS first: the workgroup's member tile [m0, m0 + MT) (blockIdx.y; MT from the LDS budget, so any M fits) holds
// overlap and member rows, tile 0 also the mask rows.  Neighbouring pixels nearly always share (member, class), so per mask
// the lane's 4 mask bits are summed across the wave from ballots (popcount of one ballot per bit of the lane's 0..4 count) and
// one lane adds the sum -- always for the mask rows, and for the overlap row when (member, class) is one value across the
// whole wave; otherwise each lane adds its own pixels (one add when its 4 pixels agree).  After a barrier the nonzero LDS words
// are added to the block in HBM with global atomicAdd (vector instructions; integer sums, so the bits do not depend on arrival
// order).  The block is zeroed on the stream before the launch.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace tsdfk {

constexpr int kAssocMaxMasks = 256;
constexpr int kAssocLdsWords = 8192;     // 32 KiB of LDS per workgroup: overlap tile + mask rows + member tile
constexpr int kAssocMaxBlocks = 256;     // workgroups per member tile (grid stride beyond)

struct AssocParams {
    const int32_t *member;       // H*W
    const float *rdepth;         // H*W
    const float *depth;          // H*W, the live frame
    const uint8_t *masks;        // K*H*W
    uint32_t *counts;            // 3KM + 3K + 4M words, zeroed
    int64_t n_px;                // H*W
    int64_t n_quads;             // ceil(H*W / 4)
    int K, M, MT;                // masks, members, members per tile
    float near_m, far_m, tol;
};

// Member tile of a workgroup: MT members from the budget after the mask rows (K <= 256 leaves at least 9).
__host__ __device__ inline int assoc_tile_members(int K, int M)
{
    const int mt = (kAssocLdsWords - 3 * K) / (3 * K + 4);
    return mt < M ? mt : M;
}

// Sum over the wave of a per-lane value in [0, 7], from one ballot per bit.
__device__ __forceinline__ uint32_t assoc_wave_sum7(uint32_t n)
{
    return (uint32_t)__popcll(__ballot(n & 1u)) + 2u * (uint32_t)__popcll(__ballot(n & 2u)) +
           4u * (uint32_t)__popcll(__ballot(n & 4u));
}

// key of a pixel in this tile: (m - m0) * 4 + class when rendered by a member of the tile, -1 otherwise.
template <bool VEC>
__global__ __launch_bounds__(256) void associate_count(AssocParams p)
{
    extern __shared__ uint32_t s_cnt[];
    const int K = p.K, MT = p.MT, m0 = blockIdx.y * MT;
    const int mt_here = min(MT, p.M - m0);
    const bool tile0 = blockIdx.y == 0;
    uint32_t *s_ov = s_cnt;                      // [K][MT][3]
    uint32_t *s_mask = s_cnt + 3 * K * MT;       // [K][3], tile 0 only
    uint32_t *s_mem = s_mask + 3 * K;            // [MT][4]
    const int words = 3 * K * MT + 3 * K + 4 * MT;
    for (int i = threadIdx.x; i < words; i += blockDim.x) s_cnt[i] = 0u;
    __syncthreads();

    const int lane = threadIdx.x & 63;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    // every lane of a wave runs the same number of iterations (the wave ops below need the whole wave): the bound is
    // rounded up to a multiple of the stride and a lane past the last quad carries no pixels
    const int64_t q_end = (p.n_quads + stride - 1) / stride * stride;
    for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < q_end; q += stride) {
        const int64_t px = 4 * q;
        int32_t mem[4] = {-1, -1, -1, -1};
        float rd[4] = {0.0f, 0.0f, 0.0f, 0.0f}, d[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        uint32_t inb = 0;                        // bit j: pixel px + j < H*W
        if (VEC) {
            if (q < p.n_quads) {
                const int4 mi = *reinterpret_cast<const int4 *>(p.member + px);
                const float4 ri = *reinterpret_cast<const float4 *>(p.rdepth + px);
                const float4 di = *reinterpret_cast<const float4 *>(p.depth + px);
                mem[0] = mi.x; mem[1] = mi.y; mem[2] = mi.z; mem[3] = mi.w;
                rd[0] = ri.x; rd[1] = ri.y; rd[2] = ri.z; rd[3] = ri.w;
                d[0] = di.x; d[1] = di.y; d[2] = di.z; d[3] = di.w;
                inb = 15u;
            }
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (px + j < p.n_px) {
                    mem[j] = p.member[px + j];
                    rd[j] = p.rdepth[px + j];
                    d[j] = p.depth[px + j];
                    inb |= 1u << j;
                }
        }
        uint32_t vbits = 0, ubits = 0;           // live valid; live valid and not rendered
        int key[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const bool in = (inb >> j) & 1u;
            const bool valid = in && __builtin_isfinite(d[j]) && p.near_m < d[j] && d[j] <= p.far_m;
            const bool rendered = in && mem[j] >= 0 && mem[j] < p.M;
            int c = 3;
            if (valid) {
                const float r = d[j] - rd[j];
                c = fabsf(r) <= p.tol ? 0 : (r < -p.tol ? 1 : 2);
            }
            vbits |= (valid ? 1u : 0u) << j;
            ubits |= (valid && !rendered ? 1u : 0u) << j;
            const int mt = mem[j] - m0;
            key[j] = rendered && mt >= 0 && mt < mt_here ? mt * 4 + c : -1;
        }
        // the lane's own pixels as one key (or -2 when they differ), and whether the whole wave has that one key (-2 in every
        // lane is no common key: each lane then adds its own pixels)
        const int lkey = key[1] == key[0] && key[2] == key[0] && key[3] == key[0] && inb == 15u ? key[0] : -2;
        const int wkey = __builtin_amdgcn_readfirstlane(lkey);
        const bool uniform = wkey != -2 && __ballot(lkey != wkey) == 0ull;
        // member rows
        if (uniform) {
            if (wkey >= 0 && lane == 0) atomicAdd(&s_mem[wkey], 256u);
        } else if (lkey >= 0) {
            atomicAdd(&s_mem[lkey], 4u);
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (key[j] >= 0) atomicAdd(&s_mem[key[j]], 1u);
        }
        // a wave with no pixel of this tile has nothing to add to it past tile 0's mask rows
        const bool any_here = __ballot(key[0] >= 0 || key[1] >= 0 || key[2] >= 0 || key[3] >= 0) != 0ull;
        if (!tile0 && !any_here) continue;
        const bool vec_mask = VEC && q < p.n_quads;
        for (int k = 0; k < K; ++k) {
            const uint8_t *mk = p.masks + (int64_t)k * p.n_px + px;
            uint32_t bits = 0;                   // bit j: pixel px + j is in mask k
            if (vec_mask) {
                const uint32_t w = *reinterpret_cast<const uint32_t *>(mk);
                bits = ((w >> 7) & 1u) | ((w >> 14) & 2u) | ((w >> 21) & 4u) | ((w >> 28) & 8u);
            } else if (!VEC) {
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if ((inb >> j) & 1u) bits |= (mk[j] >= 128 ? 1u : 0u) << j;
            }
            const uint32_t n_set = __popc(bits);
            uint32_t w_set = 0;
            if (tile0 || uniform) w_set = assoc_wave_sum7(n_set);
            if (tile0) {
                const uint32_t w_val = assoc_wave_sum7(__popc(bits & vbits));
                const uint32_t w_unx = assoc_wave_sum7(__popc(bits & ubits));
                if (lane == 0) {
                    if (w_set) atomicAdd(&s_mask[3 * k], w_set);
                    if (w_val) atomicAdd(&s_mask[3 * k + 1], w_val);
                    if (w_unx) atomicAdd(&s_mask[3 * k + 2], w_unx);
                }
            }
            if (uniform) {
                if (wkey >= 0 && (wkey & 3) != 3 && lane == 0 && w_set)
                    atomicAdd(&s_ov[(k * MT + (wkey >> 2)) * 3 + (wkey & 3)], w_set);
            } else if (lkey >= 0) {
                if ((lkey & 3) != 3 && n_set) atomicAdd(&s_ov[(k * MT + (lkey >> 2)) * 3 + (lkey & 3)], n_set);
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (((bits >> j) & 1u) && key[j] >= 0 && (key[j] & 3) != 3)
                        atomicAdd(&s_ov[(k * MT + (key[j] >> 2)) * 3 + (key[j] & 3)], 1u);
            }
        }
    }
    __syncthreads();

    // flush the nonzero words of this workgroup into the block
    const int64_t M = p.M;
    const int ov_words = 3 * K * MT;
    for (int i = threadIdx.x; i < words; i += blockDim.x) {
        const uint32_t c = s_cnt[i];
        if (c == 0u) continue;
        int64_t g;
        if (i < ov_words) {
            const int k = i / (3 * MT), r = i - k * 3 * MT;
            g = (int64_t)k * M * 3 + (int64_t)m0 * 3 + r;             // r = (m - m0) * 3 + c
        } else if (i < ov_words + 3 * K) {
            g = 3 * (int64_t)K * M + (i - ov_words);
        } else {
            g = 3 * (int64_t)K * M + 3 * K + 4 * (int64_t)m0 + (i - ov_words - 3 * K);
        }
        atomicAdd(&p.counts[g], c);
    }
}

}  // namespace tsdfk
