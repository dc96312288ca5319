// tsdf_scan.hip.h -- lidar scans: projection of a Velodyne scan to a range image, and range to z-depth.
//
// The reference's second sensor (mSensor == 1) hands Engine::Run an image of RANGES, distances along the ray, made from a
// scan on the CPU (ref: src/Utility.cpp:40-57 project, :374-419 GetRangeImageFromBinaryFile); every consumer that turns such
// a pixel into a point divides by the ray's length first (ref: src/Object.cpp:613-620, src/DoN.cpp:89-96).  Both steps are
// done here on the device, in front of everything that assumes z-depth.  All arithmetic is fp32 in the written order
// (NUMFLAGS: no contraction, correctly rounded division and square root); tests/scan_spec.py restates it in NumPy and the
// kernels match it bit for bit.  OpenCV is absent, so the reference's own functions cannot be compiled: parity is against
// the restatement of the cited lines.
//
// Projection, point i = (x, y, z, intensity) of the KITTI .bin layout, M = velo2img (3x4, row-major), image H x W:
//     h_k = ((M_k0 x + M_k1 y) + M_k2 z) + M_k3,  k = 0, 1, 2
//     reject unless h_0 >= 2                                   (ref: src/Utility.cpp:53, the reference's literal guard)
//     uf = h_0 / h_2, vf = h_1 / h_2
//     reject unless uf >= 1 && uf < (float)W && vf >= 1 && vf < (float)H
//         (float comparisons in front of any cast: NaN, infinities and h_2 <= 0 fall out here; row 0 and column 0 are never
//          written, the reference's `> 0` on the truncated integers, ref: :405)
//     u = (int)uf, v = (int)vf                                 (truncated, as cv::Point's int members are)
//     range = sqrtf((x x + y y) + z z);  reject unless range > 0                                    (ref: :407-408)
//     image[v][u] = range                                      (ref: :411; a later point overwrites an earlier one)
// "Later wins" comes out exactly whatever order the lanes run in: scan_splat takes a 64-bit unsigned maximum per pixel over
// (i + 1) << 32 | bits(range), so the key that remains is the highest index's; 0 = no point.  scan_resolve reads the key,
// writes the range and / or the depth, and puts the key back to 0: the key image is all zero again when it has run, and two
// scans through one object do not see each other.
//
// Range to depth, pixel (u, v), K = {fx, fy, cx, cy}:
//     x = ((float)u - cx) / fx,  y = ((float)v - cy) / fy,  rim = sqrtf((x x + y y) + 1)
//     d = range / rim  when range > 0 && range <= FLT_MAX,  else 0
#pragma once
#include <hip/hip_runtime.h>

#include <cfloat>
#include <cstdint>

namespace tsdfk {

struct ScanProjection {
    float m[12];     // velo2img, row-major 3x4
    int H, W;
};
struct ScanCamera { float fx, fy, cx, cy; };

constexpr int64_t kScanMaxPoints = 0xFFFFFFFFll;   // i + 1 is the key's upper word

__device__ __forceinline__ float scan_depth_of(const ScanCamera k, int u, int v, float range)
{
    const float x = ((float)u - k.cx) / k.fx;
    const float y = ((float)v - k.cy) / k.fy;
    const float rim = sqrtf((x * x + y * y) + 1.0f);
    return (range > 0.0f && range <= FLT_MAX) ? range / rim : 0.0f;
}

// The projection of point i = q into its pixel's key, the whole of the rule above: what scan_splat does for every point, and
// the selecting splat of tsdf_scan_ground.hip.h for the points it keeps.
__device__ __forceinline__ void scan_splat_point(const ScanProjection &p, const float4 q, int64_t i, unsigned long long *__restrict__ keys)
{
    const float h0 = ((p.m[0] * q.x + p.m[1] * q.y) + p.m[2] * q.z) + p.m[3];
    const float h1 = ((p.m[4] * q.x + p.m[5] * q.y) + p.m[6] * q.z) + p.m[7];
    const float h2 = ((p.m[8] * q.x + p.m[9] * q.y) + p.m[10] * q.z) + p.m[11];
    if (!(h0 >= 2.0f)) return;
    const float uf = h0 / h2, vf = h1 / h2;
    if (!(uf >= 1.0f && uf < (float)p.W && vf >= 1.0f && vf < (float)p.H)) return;
    const int u = (int)uf, v = (int)vf;          // 1 <= u < W, 1 <= v < H from here on
    const float range = sqrtf((q.x * q.x + q.y * q.y) + q.z * q.z);
    if (!(range > 0.0f)) return;
    const unsigned long long key = ((unsigned long long)(i + 1) << 32) | (unsigned long long)__float_as_uint(range);
    atomicMax(&keys[(size_t)v * p.W + u], key);
}

// One point per lane, read as one 16-byte float4 (the compiler, seeing the intensity unused, issues it as ONE 12-byte
// global_load_dwordx3 of the same address); one 8-byte atomic maximum per accepted point.
__global__ __launch_bounds__(256) void scan_splat(const ScanProjection p, const float4 *__restrict__ points, int64_t n_points,
                                                  unsigned long long *__restrict__ keys)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n_points) return;
    scan_splat_point(p, points[i], i, keys);
}

// One pixel per lane: the winning key's range into range_out and / or its depth into depth_out (either may be null), the key
// back to 0, and -- block_counts not null -- the workgroup's number of written pixels into block_counts[blockIdx.x].
__global__ __launch_bounds__(256) void scan_resolve(const ScanCamera k, int H, int W, unsigned long long *__restrict__ keys,
                                                    float *__restrict__ range_out, float *__restrict__ depth_out,
                                                    uint32_t *__restrict__ block_counts)
{
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    bool hit = false;
    if (idx < (int64_t)H * W) {
        const unsigned long long key = keys[idx];
        hit = key != 0ull;
        if (hit) keys[idx] = 0ull;
        const float range = __uint_as_float((unsigned int)(key & 0xFFFFFFFFull));
        if (range_out) range_out[idx] = range;
        if (depth_out) depth_out[idx] = scan_depth_of(k, (int)idx % W, (int)idx / W, range);
    }
    if (block_counts) {          // (uniform across the workgroup: every lane reaches the barrier)
        const int n = __syncthreads_count(hit ? 1 : 0);
        if (threadIdx.x == 0) block_counts[blockIdx.x] = (uint32_t)n;
    }
}

// The same per-pixel body for an image that already holds ranges.
__global__ __launch_bounds__(256) void scan_range_to_depth(const ScanCamera k, int H, int W, const float *__restrict__ range_in,
                                                           float *__restrict__ depth_out)
{
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (int64_t)H * W) return;
    depth_out[idx] = scan_depth_of(k, (int)idx % W, (int)idx / W, range_in[idx]);
}

}  // namespace tsdfk
