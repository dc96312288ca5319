// tsdf_extent.hip.h -- what a fused volume holds (tsdf_volume_extent, tsdf_batch_extents): the number of observed and of
// near-surface voxels, the first and second moments and the index bounds of the near-surface voxels, and how many of them
// lie against each face of the grid.  One reduction over the two arrays, 8 bytes read per voxel, nothing written to them.
//
// THE RULE.  tests/extent_spec.py restates it with exact Python integers; a constant changed here is changed there and in
// DESIGN.md ("N10") as well.  For the voxel at GLOBAL grid index (x, y, z) with TSDF t and weight w (float32):
//   observed   w > weight_thresh                       (false for a NaN weight)
//   surface    observed && fabsf(t) < band             (false for a NaN t; t == +-1 is not surface when band == 1)
// The record, integers only (so it is specified bit for bit and no order of summation can change it):
//   n_observed, n_surface          counts
//   sum[3]                         over surface voxels: x, y, z
//   sum2[6]                        xx, yy, zz, xy, xz, yz
//   border[6]                      surface voxels with x < margin; x >= dim_x - margin; then y, then z likewise, against the
//                                  GLOBAL dims.  A voxel near two faces counts for both; margin == 0 counts nothing.
//   lo[3], hi[3]                   inclusive index bounds of the surface voxels; lo = dims, hi = -1 when there are none
// A z-slab handle reports its own voxels in global z, so the records of the slabs of one grid add up (sums added, bounds by
// min / max: tsdf_extent_combine) to the record of the whole grid.  The sums are taken modulo 2^64; the host refuses a slab
// whose second moments could reach that.
//
// MAPPING.  extent_partials: grid (blocks per slice, 1, slices); the slice index goes through the batch's {member, slice}
// map, so members of different dims share one launch.  A slice is cut into wavefront tiles of 32 x 8 voxels -- a lane
// holds four x-adjacent voxels, eight lanes one 128-byte line of each array, the wavefront eight rows -- and the four
// wavefronts of a workgroup stride over the slice's tiles.  Where rows are 16-byte aligned (dim_x % 4 == 0) a lane moves
// its quad as one 16-byte load per array; otherwise (plain handles of any dim_x) every voxel is loaded on its own behind
// its bounds predicate.
// REDUCTION.  Wavefront, workgroup, one partial per workgroup:
//   * what is uniform over a tile -- the counts, the z faces, the z sums (z * k, z * z * k with k the tile's surface count)
//     and the z bounds -- comes from ballots and popcounts and lives in scalar registers;
//   * what depends on the lane -- the x and y sums, the mixed moments, the x and y faces and bounds -- is accumulated per
//     lane as 64-bit integers (a quad contributes x0 * c + o1 with c its surface count and o1 the sum of the offsets of
//     its surface voxels, and so on) and crosses the lanes ONCE per wavefront, after its last tile: integer adds and
//     integer min / max through shuffles;
//   * the four wavefronts meet in 640 bytes of LDS (4 x 17 sums, 4 x 6 bounds: the only LDS used) and the workgroup stores one 160-byte record, laid
//     out as tsdf_extent, with plain stores.  No atomics: several thousand workgroups adding 23 words to one cache line
//     would queue on it, a partial record costs one store and one load.
// extent_finish: one workgroup per member adds up the member's partial records (contiguous: the slice map is in member
// order) in a fixed order and writes the record.  Everything is integer, so the result does not depend on that order.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace tsdfk {

constexpr int kExtentWords = 20;          // 64-bit words of a record: 17 sums, then lo[3] | hi[3] as six int32
constexpr int kExtentSums = 17;           // n_observed, n_surface, sum[3], sum2[6], border[6]
constexpr int kExtentTilesPerWave = 8;    // tiles a wavefront takes before its lanes are reduced (sizes the grid)
constexpr int kExtentFinishGroups = 12;   // extent_finish: 12 groups of 20 threads, a thread per word of the record

struct ExtentVolume {
    const float *t, *w;      // the slab's arrays (slab-local z)
    int dim[3];              // GLOBAL dims
    int z_begin;             // global z of the slab's first slice
    int tiles_x, tiles;      // wavefront tiles per row of tiles / per slice
    int first_partial, n_partials;   // the member's partial records (extent_finish)
};

struct ExtentRule { float wthr, band; int margin; };

__device__ __forceinline__ unsigned long long extent_wave_sum(unsigned long long v)
{
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    return v;
}
__device__ __forceinline__ int extent_wave_min(int v)
{
    for (int off = 32; off > 0; off >>= 1) v = min(v, __shfl_xor(v, off));
    return v;
}
__device__ __forceinline__ int extent_wave_max(int v)
{
    for (int off = 32; off > 0; off >>= 1) v = max(v, __shfl_xor(v, off));
    return v;
}

// ALIGNED: dim_x % 4 == 0 (and the arrays' base is 16-byte aligned, as every allocation of the library is).
// BATCHED: the slice goes through slice_map to {member, slab-local slice} and the member's block is vols[member];
// otherwise the one volume is `one` and blockIdx.z is its slab-local slice.
template <bool ALIGNED, bool BATCHED>
__global__ __launch_bounds__(256) void extent_partials(ExtentVolume one, const ExtentVolume *vols, const int2 *slice_map,
                                                       ExtentRule R, unsigned long long *partials)
{
    typedef unsigned long long u64;
    __shared__ u64 sh_sum[4][kExtentSums];
    __shared__ int sh_bound[4][6];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int member = 0, zl = (int)blockIdx.z;
    if (BATCHED) {
        const int2 ms = slice_map[blockIdx.z];
        member = ms.x;
        zl = ms.y;
    }
    const ExtentVolume V = BATCHED ? vols[member] : one;
    const int dx = V.dim[0], dy = V.dim[1], dz = V.dim[2];
    const int z = V.z_begin + zl;
    const bool z_lo = z < R.margin, z_hi = z >= dz - R.margin;   // (dz - margin cannot overflow: dz >= 1, margin >= 0)
    // uniform over the wavefront (ballots)
    u64 n_obs = 0, n_surf = 0, s_z = 0, s_zz = 0, b_zlo = 0, b_zhi = 0;
    // per lane
    u64 s_x = 0, s_y = 0, s_xx = 0, s_yy = 0, s_xy = 0, s_xz = 0, s_yz = 0;
    unsigned int b_xlo = 0, b_xhi = 0, b_ylo = 0, b_yhi = 0;
    int lo_x = 0x7fffffff, lo_y = 0x7fffffff, hi_x = -1, hi_y = -1;
    for (int tile = (int)blockIdx.x * 4 + wave; tile < V.tiles; tile += (int)gridDim.x * 4) {   // uniform over the wavefront
        const int ty = tile / V.tiles_x, tx = tile - ty * V.tiles_x;
        const int x0 = (tx * 8 + (lane & 7)) * 4, y = ty * 8 + (lane >> 3);
        const bool row_in = x0 < dx && y < dy;
        const int64_t base = ((int64_t)zl * dy + y) * dx + x0;
        float t[4] = {1.0f, 1.0f, 1.0f, 1.0f}, w[4] = {0.0f, 0.0f, 0.0f, 0.0f};   // outside the grid: a fresh voxel, never observed
        if (ALIGNED) {
            if (row_in) {
                const float4 t4 = *reinterpret_cast<const float4 *>(V.t + base);
                const float4 w4 = *reinterpret_cast<const float4 *>(V.w + base);
                t[0] = t4.x; t[1] = t4.y; t[2] = t4.z; t[3] = t4.w;
                w[0] = w4.x; w[1] = w4.y; w[2] = w4.z; w[3] = w4.w;
            }
        } else {
#pragma unroll
            for (int v = 0; v < 4; ++v)
                if (row_in && x0 + v < dx) {
                    t[v] = V.t[base + v];
                    w[v] = V.w[base + v];
                }
        }
        unsigned int sbits = 0;    // the quad's surface voxels
        unsigned int k = 0;        // surface voxels of the tile: uniform
#pragma unroll
        for (int v = 0; v < 4; ++v) {
            // a lane outside the grid must not count even when weight_thresh < 0 lets its stand-in weight of 0 pass
            const bool obs = row_in && (ALIGNED || x0 + v < dx) && w[v] > R.wthr;
            const bool surf = obs && fabsf(t[v]) < R.band;
            n_obs += (u64)__popcll(__ballot(obs));
            k += (unsigned int)__popcll(__ballot(surf));
            sbits |= surf ? 1u << v : 0u;
        }
        if (k == 0) continue;      // uniform: nothing of this tile is near a surface
        n_surf += k;
        s_z += (u64)z * k;
        s_zz += (u64)z * (u64)z * k;
        b_zlo += z_lo ? k : 0u;
        b_zhi += z_hi ? k : 0u;
        if (sbits) {
            const unsigned int c = (unsigned int)__popc(sbits);
            const unsigned int o1 = ((sbits >> 1) & 1u) + 2u * ((sbits >> 2) & 1u) + 3u * ((sbits >> 3) & 1u);   // sum of v
            const unsigned int o2 = ((sbits >> 1) & 1u) + 4u * ((sbits >> 2) & 1u) + 9u * ((sbits >> 3) & 1u);   // sum of v * v
            const u64 X = (u64)x0, Y = (u64)y, Z = (u64)z;
            const u64 qx = X * c + o1;                 // sum of x over the quad's surface voxels
            s_x += qx;
            s_y += Y * c;
            s_xx += X * X * c + 2 * X * o1 + o2;
            s_yy += Y * Y * c;
            s_xy += Y * qx;
            s_xz += Z * qx;
            s_yz += Z * Y * c;
            // faces: voxels v < n_lo have x < margin, voxels v >= v_hi have x >= dim_x - margin (no overflow: 1 <= dx - x0 <= dx)
            const int n_lo = min(max(R.margin - x0, 0), 4), v_hi = min(max((dx - x0) - R.margin, 0), 4);
            b_xlo += (unsigned int)__popc(sbits & ((1u << n_lo) - 1u));
            b_xhi += (unsigned int)__popc(sbits & (0xfu & ~((1u << v_hi) - 1u)));
            b_ylo += y < R.margin ? c : 0u;
            b_yhi += y >= dy - R.margin ? c : 0u;
            lo_x = min(lo_x, x0 + (__ffs((int)sbits) - 1));
            hi_x = max(hi_x, x0 + (31 - __clz((int)sbits)));
            lo_y = min(lo_y, y);
            hi_y = max(hi_y, y);
        }
    }
    // across the lanes, once
    s_x = extent_wave_sum(s_x); s_y = extent_wave_sum(s_y);
    s_xx = extent_wave_sum(s_xx); s_yy = extent_wave_sum(s_yy);
    s_xy = extent_wave_sum(s_xy); s_xz = extent_wave_sum(s_xz); s_yz = extent_wave_sum(s_yz);
    const u64 f_xlo = extent_wave_sum((u64)b_xlo), f_xhi = extent_wave_sum((u64)b_xhi);
    const u64 f_ylo = extent_wave_sum((u64)b_ylo), f_yhi = extent_wave_sum((u64)b_yhi);
    lo_x = extent_wave_min(lo_x); lo_y = extent_wave_min(lo_y);
    hi_x = extent_wave_max(hi_x); hi_y = extent_wave_max(hi_y);
    if (lane == 0) {
        u64 *s = sh_sum[wave];
        s[0] = n_obs; s[1] = n_surf;
        s[2] = s_x; s[3] = s_y; s[4] = s_z;
        s[5] = s_xx; s[6] = s_yy; s[7] = s_zz; s[8] = s_xy; s[9] = s_xz; s[10] = s_yz;
        s[11] = f_xlo; s[12] = f_xhi; s[13] = f_ylo; s[14] = f_yhi; s[15] = b_zlo; s[16] = b_zhi;
        int *b = sh_bound[wave];
        b[0] = lo_x; b[1] = lo_y; b[2] = n_surf ? z : 0x7fffffff;   // a workgroup holds one slice
        b[3] = hi_x; b[4] = hi_y; b[5] = n_surf ? z : -1;
    }
    __syncthreads();
    // the workgroup's record: a thread per word
    u64 *out = partials + ((size_t)blockIdx.z * gridDim.x + blockIdx.x) * kExtentWords;
    const int i = (int)threadIdx.x;
    if (i < kExtentSums) {
        out[i] = sh_sum[0][i] + sh_sum[1][i] + sh_sum[2][i] + sh_sum[3][i];
    } else if (i < kExtentSums + 6) {
        const int j = i - kExtentSums;
        const int a = sh_bound[0][j], b = sh_bound[1][j], c = sh_bound[2][j], d = sh_bound[3][j];
        reinterpret_cast<int *>(out + kExtentSums)[j] = j < 3 ? min(min(a, b), min(c, d)) : max(max(a, b), max(c, d));
    }
}

// One workgroup of 240 threads per member: thread = (group g, word j); group g adds words j of the member's partial records
// g, g + 12, ...; the 12 groups meet in LDS.  Words 17..19 hold two int32 each: lo by min, hi by max.
template <bool BATCHED>
__global__ __launch_bounds__(kExtentFinishGroups * kExtentWords) void extent_finish(ExtentVolume one, const ExtentVolume *vols,
                                                                                    const unsigned long long *partials,
                                                                                    unsigned long long *records)
{
    typedef unsigned long long u64;
    __shared__ u64 sh[kExtentFinishGroups][kExtentWords];
    const ExtentVolume V = BATCHED ? vols[blockIdx.x] : one;
    const int g = (int)threadIdx.x / kExtentWords, j = (int)threadIdx.x - g * kExtentWords;
    const u64 *p = partials + (size_t)V.first_partial * kExtentWords;
    // words 17..19: entries e0 (low half) and e0 + 1 of {lo0, lo1, lo2, hi0, hi1, hi2}; an entry below 3 is a minimum
    const int e0 = 2 * (j - kExtentSums);
    const bool min_a = e0 < 3, min_b = e0 + 1 < 3;
    u64 sum = 0;
    int a = min_a ? 0x7fffffff : -1, b = min_b ? 0x7fffffff : -1;
    for (int i = g; i < V.n_partials; i += kExtentFinishGroups) {
        const u64 word = p[(size_t)i * kExtentWords + j];
        if (j < kExtentSums) {
            sum += word;
        } else {
            const int wa = (int)(unsigned int)word, wb = (int)(unsigned int)(word >> 32);
            a = min_a ? min(a, wa) : max(a, wa);
            b = min_b ? min(b, wb) : max(b, wb);
        }
    }
    sh[g][j] = j < kExtentSums ? sum : ((u64)(unsigned int)b << 32) | (u64)(unsigned int)a;
    __syncthreads();
    if (g != 0) return;
    u64 *out = records + (size_t)blockIdx.x * kExtentWords;
    if (j < kExtentSums) {
        u64 s = 0;
        for (int q = 0; q < kExtentFinishGroups; ++q) s += sh[q][j];
        out[j] = s;
        return;
    }
    const int d0 = V.dim[0], d1 = V.dim[1], d2 = V.dim[2];
    int r[2] = {e0 == 0 ? d0 : e0 == 2 ? d2 : -1, e0 == 0 ? d1 : -1};   // no surface voxel: lo = dims, hi = -1
    for (int q = 0; q < kExtentFinishGroups; ++q) {
        const int wa = (int)(unsigned int)sh[q][j], wb = (int)(unsigned int)(sh[q][j] >> 32);
        r[0] = min_a ? min(r[0], wa) : max(r[0], wa);
        r[1] = min_b ? min(r[1], wb) : max(r[1], wb);
    }
    out[j] = ((u64)(unsigned int)r[1] << 32) | (u64)(unsigned int)r[0];
}

}  // namespace tsdfk
