// tsdf_scan_fill.hip.h -- filling the gaps between lidar beams in a sparse z-depth image.
//
// A 64-beam scan projected into a camera image (tsdf_scan.hip.h, N14) writes a few pixels in a hundred, in rows one beam
// apart; Integrate samples the nearest pixel and skips a voxel whose pixel is empty, so such an image fuses isolated rows of
// voxels.  The fill below sits between the projection and Integrate and touches neither.  All arithmetic is fp32 in the
// written order (NUMFLAGS: no contraction, correctly rounded division, denormals kept); tests/scan_fill_spec.py restates it
// in NumPy and the kernel matches it bit for bit.
//
// Parameters: max_span_u, max_span_v in 0 ... 16 (the largest distance in pixels between two sources that is bridged; 0 or 1
// turns the pass off), jump_rel finite and >= 0.
// A SOURCE is a pixel with d > 0 && d <= FLT_MAX; everything else (0, negatives, NaN, +-inf) is EMPTY.
// One pass along a line (the image row for the u pass, the image column for the v pass), for an empty pixel:
//     da = distance to the nearest source on the low side, 1 <= da <= max_span - 1, a its value
//     db = distance to the nearest source on the high side, likewise, b its value
//         (the search stays inside the image and inside the line: a row never continues into the next one)
//     fill only if both exist, da + db <= max_span and fabsf(a - b) <= jump_rel * fminf(a, b)
//     ia = 1.0f / a;  ib = 1.0f / b;  num = ia * (float)db + ib * (float)da;  inv = num / (float)(da + db);  d = 1.0f / inv
//     d is accepted only if d > 0 && d <= FLT_MAX; otherwise, and wherever nothing is filled, the pixel keeps its input BITS
// A source always keeps its bits.  Inverse depth is what is interpolated because a plane's inverse z-depth is affine in the
// pixel coordinates: planes come out to rounding.  Nothing is extrapolated and nothing is bridged across a depth jump.
// Two passes: the u pass reads the input (its sources are measured pixels only); the v pass reads the u pass's output (its
// sources are measured and u-filled pixels, never v-filled ones).
// Kind image (uint8): 0 empty, 1 measured, 2 filled by the u pass, 3 filled by the v pass; n_filled counts kinds 2 and 3.
//
// Mapping: one kernel, one launch per image.  A workgroup of 256 lanes owns a tile of kFillTileW x kFillTileH pixels.  It
// stages the tile and a halo of max_span - 1 (at most kFillHalo) pixels on every side from HBM into LDS by coalesced row
// loads -- pixels outside the image as 0, which is empty, so the search needs no bounds of its own --, runs the u pass over
// every staged row of its own columns into a second LDS array, then the v pass over its own rows out of that array, and
// writes depth and kind.  Lanes run along u in both passes, so every LDS access is stride 1 across a wavefront.  The search
// loops are bounded by the spans, which are the same in every lane.  Input and output are different buffers: a workgroup
// reads its neighbours' pixels.
#pragma once
#include <hip/hip_runtime.h>

#include <cfloat>
#include <cstdint>

namespace tsdfk {

constexpr int kFillTileW = 64, kFillTileH = 8;         // the tile one workgroup owns: one wavefront's width by two rows a wavefront
constexpr int kFillMaxSpan = 16, kFillHalo = kFillMaxSpan - 1;
constexpr int kFillStageW = kFillTileW + 2 * kFillHalo, kFillStageH = kFillTileH + 2 * kFillHalo;    // 94 x 38
static_assert(kFillTileH % 4 == 0, "every wavefront of the four runs the same number of v-pass rounds: they hold a barrier");

struct ScanFill {
    int H, W;
    int span_u, span_v;
    float jump_rel;
};

__device__ __forceinline__ bool fill_source(float d) { return d > 0.0f && d <= FLT_MAX; }

// The pixel at *p after one pass along the line whose neighbours lie `stride` floats apart; every p[+-k * stride] with
// k < span is staged.
__device__ __forceinline__ float fill_pixel(const float *p, int stride, int span, float jump_rel)
{
    const float x = *p;
    int da = 0, db = 0;
    float a = 0.0f, b = 0.0f;
    for (int k = 1; k < span; ++k) {
        const float lo = p[-k * stride], hi = p[k * stride];
        if (da == 0 && fill_source(lo)) { da = k; a = lo; }
        if (db == 0 && fill_source(hi)) { db = k; b = hi; }
    }
    if (fill_source(x) || da == 0 || db == 0 || da + db > span) return x;
    if (!(fabsf(a - b) <= jump_rel * fminf(a, b))) return x;
    const float ia = 1.0f / a, ib = 1.0f / b;
    const float num = ia * (float)db + ib * (float)da;
    const float inv = num / (float)(da + db);
    const float d = 1.0f / inv;
    return fill_source(d) ? d : x;
}

// grid (ceil(W / kFillTileW), ceil(H / kFillTileH)); kind and block_counts may be null.  block_counts[blockIdx.y * gridDim.x +
// blockIdx.x] = the tile's number of filled pixels inside the image.
__global__ __launch_bounds__(256) void scan_fill(const ScanFill f, const float *__restrict__ in, float *__restrict__ out,
                                                 uint8_t *__restrict__ kind, uint32_t *__restrict__ block_counts)
{
    __shared__ float s_in[kFillStageH][kFillStageW];     // the input: the tile and its halo
    __shared__ float s_u[kFillStageH][kFillTileW];       // the u pass's output: the tile's columns, every staged row
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int hu = min(max(f.span_u - 1, 0), kFillHalo), hv = min(max(f.span_v - 1, 0), kFillHalo);
    const int u0 = (int)blockIdx.x * kFillTileW, v0 = (int)blockIdx.y * kFillTileH;
    const int rows = kFillTileH + 2 * hv, cols = kFillTileW + 2 * hu;

    for (int r = wave; r < rows; r += 4) {
        const int v = v0 - hv + r;
        const bool row_inside = v >= 0 && v < f.H;
        for (int c = lane; c < cols; c += 64) {
            const int u = u0 - hu + c;
            float d = 0.0f;
            if (row_inside && u >= 0 && u < f.W) d = in[(int64_t)v * f.W + u];
            s_in[r][c] = d;
        }
    }
    __syncthreads();
    for (int r = wave; r < rows; r += 4) s_u[r][lane] = fill_pixel(&s_in[r][lane + hu], 1, hu + 1, f.jump_rel);
    __syncthreads();
    uint32_t n_filled = 0;
    for (int r = wave; r < kFillTileH; r += 4) {         // (the same rounds in every wavefront: every lane reaches the barriers)
        const int u = u0 + lane, v = v0 + r;
        const float x = s_in[r + hv][lane + hu], xu = s_u[r + hv][lane];
        const float xv = fill_pixel(&s_u[r + hv][lane], kFillTileW, hv + 1, f.jump_rel);
        const int k = fill_source(x) ? 1 : fill_source(xu) ? 2 : fill_source(xv) ? 3 : 0;
        const bool inside = u < f.W && v < f.H;
        if (inside) {
            const int64_t idx = (int64_t)v * f.W + u;
            out[idx] = xv;
            if (kind) kind[idx] = (uint8_t)k;
        }
        if (block_counts) n_filled += (uint32_t)__syncthreads_count(inside && k >= 2 ? 1 : 0);
    }
    if (block_counts && threadIdx.x == 0) block_counts[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = n_filled;
}

}  // namespace tsdfk
