// tsdf_segment.hip.h -- geometric segmentation of a depth frame (difference of normals, then clustering) and the refinement
// of instance masks by the clusters: the kernels of tsdf_segment_depth_device / tsdf_segment_refine_masks_device /
// tsdf_segment_frame (the host side is in tsdf_capi.hip).  It stands in for the reference's DoN extractor and fuse_segments
// (ref: src/DoN.cpp:129-270, src/Engine.cpp:300-338), which are a PCL pipeline on the CPU.
//
// THE RULE.  Every operation is correctly rounded (float32 and double + - * / sqrt in the order written -- the library builds
// with -ffp-contract=off, csrc/Makefile NUMFLAGS -- comparisons, integer arithmetic) and every sum is an integer sum, so
// tests/segment_spec.py, which restates the rule in NumPy, gives the same bits.  A change here is a change there and in
// include/tsdf_hip.h and DESIGN.md ("N8 -- geometric segmentation") as well.
//
//   Points   pixel p = (u, v), d = depth[p], is valid iff isfinite(d) && near_m < d && d <= far_m.  Its point, float32:
//            x = (u - cx) / fx * d, y = (v - cy) / fy * d, z = d; each coordinate c becomes the int32
//            clamp(rintf(c * 8192.0f), -2^29, 2^29): quanta of 2^-13 m.  far_m <= 32.  P is the point of p, Q of a tap.
//   Normal   at radius r (0 < r <= 32 m), R = rintf(r * 8192.0f).  The window is the lattice of (2T + 1)^2 taps, T = 8: tap
//            (i, j), -T <= i, j <= T, reads pixel (u + i * sx, v + j * sy), sx = (hx + T - 1) / T (integer division) with
//            hx = (int)fminf(fmaxf(floorf(fx * r / d), 1), W); sy, hy the same from fy and H.  A tap counts iff it is inside
//            the image, valid, and |Q - P|^2 <= R^2 in int64 (a true 3-D gate; the centre tap always counts).
//            Over the counted taps, D = Q - P: n, S1[a] = sum D_a, S2[ab] = sum D_a D_b as integers.  In double:
//            m_a = S1[a] / n, cov_ab = S2[ab] / n - m_a * m_b.  kSegSweeps = 5 cyclic Jacobi sweeps, each rotating (0,1), (0,2),
//            (1,2): a rotation with a_pq == 0 is skipped, otherwise theta = (a_qq - a_pp) / (2 a_pq),
//            t = (theta >= 0 ? 1 : -1) / (|theta| + sqrt(theta * theta + 1)), c = 1 / sqrt(t * t + 1), s = t * c,
//            a_pp -= t a_pq, a_qq += t a_pq, a_pq = 0, (a_rp, a_rq) = (c a_rp - s a_rq, s a_rp + c a_rq), and the same pair
//            update on columns p, q of V (V starts as the identity).  (5 sweeps agree with LAPACK to 8e-16 of the largest
//            eigenvalue on random matrices.)  The normal is V's column of the smallest diagonal entry (ties to the lower
//            index), negated when (n_x P_x + n_y P_y) + n_z P_z > 0: it faces the camera.
//            There is a normal iff the pixel is valid, n >= 3 and the middle diagonal entry is > 1.0 -- one squared
//            quantum: the spread rounding alone gives collinear points stays below that, a surface patch is far above.
//   DoN      don = 0.5 * sqrt((dx dx + dy dy) + dz dz) of n_small - n_large, double.  A pixel is kept iff both normals exist
//            and don > (double)don_thresh.  The image holds (float)don, 0 where a normal is missing.
//   Cluster  kept 4-neighbours are joined iff |P - Q|^2 <= rintf(seg_radius * 8192)^2.  A component of fewer than
//            min_cluster or more than max_cluster pixels is dropped; the others are numbered 1..C by their smallest flat
//            pixel index.  The cluster image is int32, 0 = none.
//   Refine   masks: K contiguous H * W byte images.  in(k, p): byte >= 128.  deep(k, p): in(k, q) for every q of the
//            (2 inset + 1)^2 square around p, q outside the image counting as not in.  A pixel is labelled iff its cluster
//            value c is in 1..C.  uint32 counts, one block of C + C K words: size[c] at c - 1, inside[c][k] = #{p labelled c:
//            deep(k, p)} at C + (c - 1) K + k.  accept(c, k) iff (float)inside / (float)size > overlap (float32, strict;
//            ref: src/Engine.cpp:322-325).  out[k][p] = 255 iff p is labelled c, deep(k, p) and accept(c, k); else 0.
//
// MAPPING.  seg_backproject: a lane per pixel writes {x, y, z, bits of d or 0} as one 16-byte store (4.9 MB at 640 x 480, it
// stays in L2 / Infinity Cache for the gathers).  seg_don: a 16 x 16 pixel tile per 256-lane workgroup, every lane walks the
// 289 taps of both radii with clamped (always in-bounds) 16-byte gathers and predicated integer accumulation -- differences
// fit int32, so products are v_mad_i64_i32 -- then the double part in registers; it also writes parent[p] = p (kept) or -1.
// seg_merge: a lane per kept pixel unites it with its right and lower neighbour: find follows parent[] with relaxed
// device-scope loads, the larger root is linked to the smaller by a vector atomicMin, retried until it lands on a root, so
// every root is its component's smallest index whatever the order.  seg_root_size writes root[p] and counts sizes (lanes of
// a wave that share a root add once).  seg_block_count / seg_scan_blocks / seg_number give the roots that pass the size
// filter their rank in flat order (ballot ranks, one workgroup scans the block sums), seg_label writes the cluster image.
// seg_refine_count: blockIdx.y = mask; a lane per pixel tests the window of a labelled pixel only, writes deep as 255 / 0
// into the output and adds to size / inside -- summed across the wave per distinct cluster first, then a global atomicAdd
// (vector instructions; integer sums).  seg_refine_accept clears the output pixels whose (cluster, mask) is not accepted.
// No load or store leaves its image: neighbour and tap coordinates are tested or clamped before they address memory, and a
// cluster value only addresses the count block after 1 <= c <= C.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace tsdfk {

constexpr int kSegTaps = 8;              // T
constexpr int kSegSweeps = 5;
constexpr int kSegMaxInset = 16;
constexpr int kSegQuantClamp = 1 << 29;

struct SegCamera {
    float fx, fy, cx, cy;
    float near_m, far_m;
    int H, W;
};

__device__ __forceinline__ int seg_quant(float c)
{
    const float q = rintf(c * 8192.0f);
    return (int)fminf(fmaxf(q, -(float)kSegQuantClamp), (float)kSegQuantClamp);
}

__global__ __launch_bounds__(256) void seg_backproject(SegCamera k, const float *__restrict__ depth, int4 *__restrict__ pts)
{
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= (int64_t)k.H * k.W) return;
    const int v = (int)(p / k.W), u = (int)(p - (int64_t)v * k.W);
    const float d = depth[p];
    int4 o = make_int4(0, 0, 0, 0);
    if (__builtin_isfinite(d) && k.near_m < d && d <= k.far_m) {
        const float x = ((float)u - k.cx) / k.fx * d;
        const float y = ((float)v - k.cy) / k.fy * d;
        o = make_int4(seg_quant(x), seg_quant(y), seg_quant(d), __float_as_int(d));   // d > 0: its bits are never 0
    }
    pts[p] = o;
}

template <int P, int Q>
__device__ __forceinline__ void seg_rotate(double &app, double &aqq, double &apq, double &arp, double &arq, double (&V)[3][3])
{
    if (apq == 0.0) return;
    const double theta = (aqq - app) / (2.0 * apq);
    const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
    const double c = 1.0 / sqrt(t * t + 1.0);
    const double s = t * c;
    const double tap = t * apq;
    app = app - tap;
    aqq = aqq + tap;
    const double nrp = c * arp - s * arq, nrq = s * arp + c * arq;
    arp = nrp;
    arq = nrq;
    apq = 0.0;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const double vp = c * V[k][P] - s * V[k][Q], vq = s * V[k][P] + c * V[k][Q];
        V[k][P] = vp;
        V[k][Q] = vq;
    }
}

__device__ __forceinline__ int seg_step(float focal_r, float d, int size)
{
    const int h = (int)fminf(fmaxf(floorf(focal_r / d), 1.0f), (float)size);
    return (h + kSegTaps - 1) / kSegTaps;
}

// The normal of valid pixel (u, v) with point P at radius r; false when there is none.
__device__ __forceinline__ bool seg_normal(const int4 *__restrict__ pts, const SegCamera &k, int u, int v, int4 P, float r,
                                           double n_out[3])
{
    const float d = __int_as_float(P.w);
    const int sx = seg_step(k.fx * r, d, k.W), sy = seg_step(k.fy * r, d, k.H);
    const int64_t R = (int64_t)rintf(r * 8192.0f), R2 = R * R;
    int n = 0, s1x = 0, s1y = 0, s1z = 0;         // |D| <= R <= 2^18 for a counted tap: 289 of them fit int32
    int64_t sxx = 0, sxy = 0, sxz = 0, syy = 0, syz = 0, szz = 0;
    for (int j = -kSegTaps; j <= kSegTaps; ++j) {
        const int vv = v + j * sy;
        const bool row_in = vv >= 0 && vv < k.H;
        const int4 *row = pts + (int64_t)min(max(vv, 0), k.H - 1) * k.W;
#pragma unroll
        for (int i = -kSegTaps; i <= kSegTaps; ++i) {
            const int uu = u + i * sx;
            const int4 Q = row[min(max(uu, 0), k.W - 1)];
            int dx = Q.x - P.x, dy = Q.y - P.y, dz = Q.z - P.z;
            const int64_t dist2 = (int64_t)dx * dx + (int64_t)dy * dy + (int64_t)dz * dz;
            const bool cnt = row_in && uu >= 0 && uu < k.W && Q.w != 0 && dist2 <= R2;
            dx = cnt ? dx : 0;
            dy = cnt ? dy : 0;
            dz = cnt ? dz : 0;
            n += cnt ? 1 : 0;
            s1x += dx; s1y += dy; s1z += dz;
            sxx += (int64_t)dx * dx; sxy += (int64_t)dx * dy; sxz += (int64_t)dx * dz;
            syy += (int64_t)dy * dy; syz += (int64_t)dy * dz; szz += (int64_t)dz * dz;
        }
    }
    const double nn = (double)n;                  // >= 1: the centre tap
    const double mx = (double)s1x / nn, my = (double)s1y / nn, mz = (double)s1z / nn;
    double a00 = (double)sxx / nn - mx * mx, a01 = (double)sxy / nn - mx * my, a02 = (double)sxz / nn - mx * mz;
    double a11 = (double)syy / nn - my * my, a12 = (double)syz / nn - my * mz, a22 = (double)szz / nn - mz * mz;
    double V[3][3] = {{1.0, 0.0, 0.0}, {0.0, 1.0, 0.0}, {0.0, 0.0, 1.0}};
    for (int sweep = 0; sweep < kSegSweeps; ++sweep) {
        seg_rotate<0, 1>(a00, a11, a01, a02, a12, V);
        seg_rotate<0, 2>(a00, a22, a02, a01, a12, V);
        seg_rotate<1, 2>(a11, a22, a12, a01, a02, V);
    }
    int col = 0;
    double lmin = a00;
    if (a11 < lmin) { col = 1; lmin = a11; }
    if (a22 < lmin) col = 2;
    const double lo01 = a11 < a00 ? a11 : a00, hi01 = a11 < a00 ? a00 : a11;
    const double mid = a22 < lo01 ? lo01 : (a22 < hi01 ? a22 : hi01);
    double nx = col == 0 ? V[0][0] : (col == 1 ? V[0][1] : V[0][2]);
    double ny = col == 0 ? V[1][0] : (col == 1 ? V[1][1] : V[1][2]);
    double nz = col == 0 ? V[2][0] : (col == 1 ? V[2][1] : V[2][2]);
    const double dot = (nx * (double)P.x + ny * (double)P.y) + nz * (double)P.z;
    if (dot > 0.0) { nx = -nx; ny = -ny; nz = -nz; }
    n_out[0] = nx; n_out[1] = ny; n_out[2] = nz;
    return n >= 3 && mid > 1.0;
}

// don (may be null) and parent: p where the pixel is kept, -1 elsewhere.
__global__ __launch_bounds__(256) void seg_don(SegCamera k, const int4 *__restrict__ pts, float r_small, float r_large,
                                               float don_thresh, float *__restrict__ don, int32_t *__restrict__ parent)
{
    const int u = blockIdx.x * 16 + (threadIdx.x & 15), v = blockIdx.y * 16 + (threadIdx.x >> 4);
    if (u >= k.W || v >= k.H) return;
    const int64_t p = (int64_t)v * k.W + u;
    const int4 P = pts[p];
    double val = 0.0;
    bool both = false;
    if (P.w != 0) {
        double ns[3], nl[3];
        const bool es = seg_normal(pts, k, u, v, P, r_small, ns);
        const bool el = seg_normal(pts, k, u, v, P, r_large, nl);
        both = es && el;
        if (both) {
            const double dx = ns[0] - nl[0], dy = ns[1] - nl[1], dz = ns[2] - nl[2];
            val = 0.5 * sqrt((dx * dx + dy * dy) + dz * dz);
        }
    }
    if (don) don[p] = (float)val;
    parent[p] = both && val > (double)don_thresh ? (int32_t)p : -1;
}

__device__ __forceinline__ int32_t seg_load(const int32_t *a) { return __hip_atomic_load(a, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// The root of kept pixel a: parent[] never increases and parent[x] <= x, so the walk ends.
__device__ __forceinline__ int32_t seg_find(const int32_t *parent, int32_t a)
{
    int32_t n;
    while ((n = seg_load(parent + a)) != a) a = n;
    return a;
}

__device__ __forceinline__ void seg_unite(int32_t *parent, int32_t a, int32_t b)
{
    bool done = false;
    while (!done) {
        a = seg_find(parent, a);
        b = seg_find(parent, b);
        if (a == b) break;
        if (a < b) { const int32_t t = a; a = b; b = t; }       // a > b: link a under b
        const int32_t old = atomicMin(parent + a, b);
        done = old == a;                                         // a was still a root: linked
        a = old;                                                 // otherwise somebody linked a first: go on from there
    }
}

__device__ __forceinline__ bool seg_joined(int4 A, int4 B, int64_t R2)
{
    const int dx = A.x - B.x, dy = A.y - B.y, dz = A.z - B.z;
    return (int64_t)dx * dx + (int64_t)dy * dy + (int64_t)dz * dz <= R2;
}

__global__ __launch_bounds__(256) void seg_merge(int H, int W, const int4 *__restrict__ pts, int64_t R2, int32_t *parent)
{
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= (int64_t)H * W) return;
    if (seg_load(parent + p) < 0) return;
    const int v = (int)(p / W), u = (int)(p - (int64_t)v * W);
    const int4 P = pts[p];
    if (u + 1 < W && seg_load(parent + p + 1) >= 0 && seg_joined(P, pts[p + 1], R2)) seg_unite(parent, (int32_t)p, (int32_t)p + 1);
    if (v + 1 < H && seg_load(parent + p + W) >= 0 && seg_joined(P, pts[p + W], R2)) seg_unite(parent, (int32_t)p, (int32_t)(p + W));
}

// Adds, for every distinct key >= 0 among the lanes of the wave, the number of lanes holding it to base[key]: one atomic per
// distinct key.  Every lane of the wave must call it (a lane with nothing to add passes -1).
__device__ __forceinline__ void seg_wave_add(uint32_t *base, int key)
{
    const int lane = threadIdx.x & 63;
    bool pending = key >= 0;
    for (;;) {
        const unsigned long long m = __ballot(pending);
        if (m == 0ull) break;
        const int leader = __ffsll((long long)m) - 1;
        const int k0 = __shfl(key, leader);
        const bool mine = pending && key == k0;
        const unsigned long long same = __ballot(mine);
        if (mine) {
            if (lane == leader) atomicAdd(base + k0, (uint32_t)__popcll(same));
            pending = false;
        }
    }
}

// root[p] = the root of a kept pixel or -1; size[root] += 1 (size zeroed before).
__global__ __launch_bounds__(256) void seg_root_size(int64_t n_px, const int32_t *__restrict__ parent, int32_t *__restrict__ root,
                                                     uint32_t *size)
{
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    int32_t r = -1;
    if (p < n_px) {
        if (parent[p] >= 0) r = seg_find(parent, (int32_t)p);
        root[p] = r;
    }
    seg_wave_add(size, r);
}

__device__ __forceinline__ bool seg_is_numbered(int64_t p, int64_t n_px, const int32_t *root, const uint32_t *size, uint32_t lo,
                                                uint32_t hi)
{
    if (p >= n_px || root[p] != (int32_t)p) return false;
    const uint32_t s = size[p];
    return s >= lo && s <= hi;
}

__global__ __launch_bounds__(256) void seg_block_count(int64_t n_px, const int32_t *__restrict__ root, const uint32_t *__restrict__ size,
                                                       uint32_t lo, uint32_t hi, uint32_t *__restrict__ blocks)
{
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int c = __syncthreads_count(seg_is_numbered(p, n_px, root, size, lo, hi) ? 1 : 0);
    if (threadIdx.x == 0) blocks[blockIdx.x] = (uint32_t)c;
}

// One workgroup: blocks[] becomes its exclusive prefix sum, *total the sum.
__global__ __launch_bounds__(1024) void seg_scan_blocks(uint32_t *blocks, int n_blocks, int32_t *total)
{
    __shared__ uint32_t s[1024];
    uint32_t carry = 0;
    for (int base = 0; base < n_blocks; base += 1024) {
        const int i = base + (int)threadIdx.x;
        const uint32_t x = i < n_blocks ? blocks[i] : 0u;
        s[threadIdx.x] = x;
        __syncthreads();
        for (int off = 1; off < 1024; off <<= 1) {
            const uint32_t add = threadIdx.x >= (unsigned)off ? s[threadIdx.x - off] : 0u;
            __syncthreads();
            s[threadIdx.x] += add;
            __syncthreads();
        }
        if (i < n_blocks) blocks[i] = carry + s[threadIdx.x] - x;
        carry += s[1023];
        __syncthreads();
    }
    if (threadIdx.x == 0) *total = (int32_t)carry;
}

// num[p] = the number (1..C) of a root that passes the size filter; other entries are not written.
__global__ __launch_bounds__(256) void seg_number(int64_t n_px, const int32_t *__restrict__ root, const uint32_t *__restrict__ size,
                                                  uint32_t lo, uint32_t hi, const uint32_t *__restrict__ blocks, int32_t *__restrict__ num)
{
    __shared__ uint32_t s_wave[4];
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const bool f = seg_is_numbered(p, n_px, root, size, lo, hi);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned long long m = __ballot(f);
    if (lane == 0) s_wave[wave] = (uint32_t)__popcll(m);
    __syncthreads();
    if (!f) return;
    uint32_t rank = blocks[blockIdx.x] + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
    for (int w = 0; w < wave; ++w) rank += s_wave[w];
    num[p] = (int32_t)rank + 1;
}

__global__ __launch_bounds__(256) void seg_label(int64_t n_px, const int32_t *__restrict__ root, const uint32_t *__restrict__ size,
                                                 uint32_t lo, uint32_t hi, const int32_t *__restrict__ num, int32_t *__restrict__ cluster)
{
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= n_px) return;
    const int32_t r = root[p];
    int32_t c = 0;
    if (r >= 0) {
        const uint32_t s = size[r];
        if (s >= lo && s <= hi) c = num[r];
    }
    cluster[p] = c;
}

struct SegRefine {
    const int32_t *cluster;      // H*W
    const uint8_t *masks;        // K*H*W
    uint8_t *out;                // K*H*W
    uint32_t *counts;            // C + C*K words (zeroed before seg_refine_count)
    int H, W, K, C, inset;
    float overlap;
};

__global__ __launch_bounds__(256) void seg_refine_count(SegRefine a)
{
    const int64_t n_px = (int64_t)a.H * a.W;
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int k = blockIdx.y;
    int c = 0;
    bool deep = false;
    if (p < n_px) {
        c = a.cluster[p];
        if (c < 1 || c > a.C) c = 0;
        if (c) {
            const int v = (int)(p / a.W), u = (int)(p - (int64_t)v * a.W);
            deep = u - a.inset >= 0 && u + a.inset < a.W && v - a.inset >= 0 && v + a.inset < a.H;
            const uint8_t *m = a.masks + (int64_t)k * n_px;
            for (int dy = -a.inset; deep && dy <= a.inset; ++dy)
                for (int dx = -a.inset; dx <= a.inset; ++dx)
                    if (m[p + (int64_t)dy * a.W + dx] < 128) { deep = false; break; }
        }
        a.out[(int64_t)k * n_px + p] = deep ? 255 : 0;
    }
    if (k == 0) seg_wave_add(a.counts, c ? c - 1 : -1);
    seg_wave_add(a.counts + a.C, deep ? (c - 1) * a.K + k : -1);
}

__global__ __launch_bounds__(256) void seg_refine_accept(SegRefine a)
{
    const int64_t n_px = (int64_t)a.H * a.W;
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int k = blockIdx.y;
    if (p >= n_px) return;
    uint8_t *o = a.out + (int64_t)k * n_px + p;
    if (*o == 0) return;
    const int c = a.cluster[p];                  // 1..C: seg_refine_count wrote 255 for such pixels only
    const float frac = (float)a.counts[a.C + (int64_t)(c - 1) * a.K + k] / (float)a.counts[c - 1];
    if (!(frac > a.overlap)) *o = 0;
}

}  // namespace tsdfk
