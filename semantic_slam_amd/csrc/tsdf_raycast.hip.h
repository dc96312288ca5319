// tsdf_raycast.hip.h -- rendering a fused volume from a camera: depth, normal, label and colour images (tsdf_raycast*).
//
// THE RULE.  Every operation is float32 and is evaluated in the order written (the library builds with -ffp-contract=off and
// IEEE division and sqrt, csrc/Makefile NUMFLAGS), so tests/raycast_spec.py, which restates it in float32 NumPy, matches the
// device bit for bit.  A constant changed here is changed there and in DESIGN.md ("Raycasting") as well.
//
//   Pose    cam2base = inverse(base2world) * cam2world, composed on the host as Integrate composes it (compose_cam2base);
//           R = its rotation (row-major), T = its translation.
//   Ray     pixel (u, v), integer coordinates:  dcx = ((float)u - cx) / fx,  dcy = ((float)v - cy) / fy;
//           db_i = (R_i0 * dcx + R_i1 * dcy) + R_i2   (the base-frame direction per unit camera z);
//           go_i = (T_i - origin_i) / vs (host),  gd_i = db_i / vs;  the sample at camera depth t is g_i = go_i + t * gd_i
//           (grid units, voxel centres at integers).  t IS camera z, so the depth output is t itself.
//           r = 1 / sqrtf((dcx * dcx + dcy * dcy) + 1) turns a step in space into a step in t.
//           A ray with a go_i or gd_i that is not finite is a miss.
//   Box     slab method against [0, dim_i - 1] (hi_i = (float)(dim_i - 1)), t_enter = near, t_exit = far, then per axis:
//           gd_i == 0: a miss unless 0 <= go_i <= hi_i (the ray is always or never inside on that axis);
//           otherwise a = (0 - go_i) / gd_i, b = (hi_i - go_i) / gd_i, lo = a < b ? a : b, up = a < b ? b : a,
//           t_enter = lo > t_enter ? lo : t_enter, t_exit = up < t_exit ? up : t_exit.
//           !(t_enter <= t_exit) is a miss.  (Comparisons rather than fmaxf / fminf: the choice between +0 and -0 stays defined.)
//   Sample  valid iff every g_i is in [0, hi_i], all 8 corner weights are > weight_thresh, and F is finite.
//           j_i = min((int)floorf(g_i), dim_i - 2), f_i = g_i - (float)j_i; corner values c_xyz = tsdf at j + (x, y, z);
//           a_yz = c_0yz + f_0 * (c_1yz - c_0yz) for yz = 00, 10, 01, 11;  b_z = a_0z + f_1 * (a_1z - a_0z);
//           F = b_0 + f_2 * (b_1 - b_0).
//           (Finite, not merely "not NaN": an infinite F would make the hit depth below inf / inf.)
//   March   t = t_enter; at most max_steps = 2 * (dim_x + dim_y + dim_z) + 8 samples.  After a sample that is not a hit:
//           step (metres) = fmaxf(vs, s_free * F) if valid and F > 0;  vs if valid and F <= 0;  s_free if invalid;
//           s_free = 0.8f * trunc (host).  t' = t + step * r.  !(t' > t) ends the march as a miss; otherwise t = t' and
//           !(t <= t_exit) ends it as a miss.  The cap and the strict increase make every lane finish (a lane that could spin
//           would hang a shared machine); a march that reaches the cap is a miss.
//   Hit     two consecutive valid samples k-1, k with F_{k-1} > 0 and F_k <= 0:
//           t* = t_{k-1} + (t_k - t_{k-1}) * (F_{k-1} / (F_{k-1} - F_k)).  depth = t*.
//   Normal  g*_i = go_i + t* * gd_i;  n_i = F(g* + e_i) - F(g* - e_i) (g*_i +- 1.0f on axis i only), six samples, any of them
//           invalid: normal (0, 0, 0).  Camera frame: m_j = (R_0j * n_0 + R_1j * n_1) + R_2j * n_2;
//           len = sqrtf((m_0 * m_0 + m_1 * m_1) + m_2 * m_2); unless len is finite and > 0 the normal is (0, 0, 0),
//           else m_j / len.  It points toward increasing TSDF, i.e. toward the camera.
//   Label / colour   the voxel clamp(floorf(g*_i + 0.5f), 0, hi_i) (float comparisons, then int); its fused uint16 label or
//           packed uint32 colour.
//   Miss    depth 0, normal (0, 0, 0), label 0, colour 0; member -1 in a batch render.
//   Batch   per pixel the member with the smallest t* wins, ties to the lower index; a member whose t_enter is not below the
//           best t* so far cannot win (t* >= t_{k-1} >= t_enter) and is not marched.
//
// MAPPING.  One ray per lane; a wavefront covers an 8 x 8 pixel tile, so neighbouring rays gather neighbouring cells through
// L1 / L2; a 256-thread workgroup covers 16 x 16 pixels.  No LDS, no barrier: a lane outside the image returns at once.  The
// hardware texture filter is not used: its weights are low-precision fixed point and would not reproduce F.  Every gather is
// bounds-safe by construction: a sample is only loaded after g has been checked to lie in [0, hi] on every axis, so
// j_i in [0, dim_i - 2] and j_i + 1 <= dim_i - 1; the label / colour voxel is clamped into the grid.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace tsdfk {

// One volume as the march sees it (a whole grid; slab handles are refused on the host).
struct RayVolume {
    const float *tsdf;
    const float *weight;
    float r[9];          // rotation of cam2base, row-major
    float go[3];         // (T - origin) / vs
    float hi[3];         // dim_i - 1
    float vs, s_free;
    int dim[3];
    int max_steps;
};

struct RaycastParams {
    RayVolume vol;
    const uint16_t *label;      // fused labels (or null when no label image is wanted)
    const uint32_t *colour;     // fused colours (likewise)
    float *depth;               // H*W          (each output may be null)
    float *normal;              // H*W*3
    uint16_t *label_out;        // H*W
    uint32_t *colour_out;       // H*W
    float fx, fy, cx, cy, near_m, far_m, wthr;
    int H, W;
};

struct BatchRaycastParams {
    const RayVolume *members;   // n members in HBM
    int n;
    float *depth, *normal;
    int32_t *member;
    float fx, fy, cx, cy, near_m, far_m, wthr;
    int H, W;
};

// F at g, when the sample is valid (see the rule).
__device__ __forceinline__ bool ray_sample(const RayVolume &V, float wthr, float g0, float g1, float g2, float &F)
{
    if (!(g0 >= 0.0f && g0 <= V.hi[0] && g1 >= 0.0f && g1 <= V.hi[1] && g2 >= 0.0f && g2 <= V.hi[2])) return false;
    const int j0 = min((int)floorf(g0), V.dim[0] - 2);
    const int j1 = min((int)floorf(g1), V.dim[1] - 2);
    const int j2 = min((int)floorf(g2), V.dim[2] - 2);
    const float f0 = g0 - (float)j0, f1 = g1 - (float)j1, f2 = g2 - (float)j2;
    const int64_t sy = V.dim[0], sz = (int64_t)V.dim[0] * V.dim[1];
    const int64_t b = (int64_t)j2 * sz + (int64_t)j1 * sy + j0;
    const float *t = V.tsdf + b, *w = V.weight + b;
    const float c000 = t[0], c100 = t[1], c010 = t[sy], c110 = t[sy + 1];
    const float c001 = t[sz], c101 = t[sz + 1], c011 = t[sz + sy], c111 = t[sz + sy + 1];
    const bool wok = w[0] > wthr && w[1] > wthr && w[sy] > wthr && w[sy + 1] > wthr &&
                     w[sz] > wthr && w[sz + 1] > wthr && w[sz + sy] > wthr && w[sz + sy + 1] > wthr;
    const float a00 = c000 + f0 * (c100 - c000);
    const float a10 = c010 + f0 * (c110 - c010);
    const float a01 = c001 + f0 * (c101 - c001);
    const float a11 = c011 + f0 * (c111 - c011);
    const float b0 = a00 + f1 * (a10 - a00);
    const float b1 = a01 + f1 * (a11 - a01);
    F = b0 + f2 * (b1 - b0);
    return wok && __builtin_isfinite(F);
}

// Direction of the ray in grid units (gd) and its clipped t range; false = a miss.
__device__ __forceinline__ bool ray_setup(const RayVolume &V, float dcx, float dcy, float near_m, float far_m, float gd[3],
                                          float &t_enter, float &t_exit)
{
    bool ok = true;
    t_enter = near_m;
    t_exit = far_m;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const float db = (V.r[3 * i] * dcx + V.r[3 * i + 1] * dcy) + V.r[3 * i + 2];
        gd[i] = db / V.vs;
        const float go = V.go[i];
        ok = ok && __builtin_isfinite(go) && __builtin_isfinite(gd[i]);
        if (gd[i] == 0.0f) {
            ok = ok && go >= 0.0f && go <= V.hi[i];
        } else {
            const float a = (0.0f - go) / gd[i], b = (V.hi[i] - go) / gd[i];
            const float lo = a < b ? a : b, up = a < b ? b : a;
            t_enter = lo > t_enter ? lo : t_enter;
            t_exit = up < t_exit ? up : t_exit;
        }
    }
    return ok && t_enter <= t_exit;
}

// The march of one ray from t_enter; true = a hit at *t_hit.
__device__ __forceinline__ bool ray_march(const RayVolume &V, float wthr, const float gd[3], float r, float t_enter,
                                          float t_exit, float *t_hit)
{
    float t = t_enter, t_prev = 0.0f, F_prev = 0.0f;
    bool prev_valid = false;
    for (int k = 0; k < V.max_steps; ++k) {
        float F = 0.0f;
        const bool valid = ray_sample(V, wthr, V.go[0] + t * gd[0], V.go[1] + t * gd[1], V.go[2] + t * gd[2], F);
        if (valid && prev_valid && F_prev > 0.0f && F <= 0.0f) {
            *t_hit = t_prev + (t - t_prev) * (F_prev / (F_prev - F));
            return true;
        }
        const float step = valid ? (F > 0.0f ? fmaxf(V.vs, V.s_free * F) : V.vs) : V.s_free;
        const float tn = t + step * r;
        if (!(tn > t)) return false;
        t_prev = t;
        F_prev = F;
        prev_valid = valid;
        t = tn;
        if (!(t <= t_exit)) return false;
    }
    return false;
}

// Camera-frame unit normal at the hit; false (and zeros) when a central difference is not available.
__device__ __forceinline__ bool ray_normal(const RayVolume &V, float wthr, const float g[3], float m[3])
{
    float n[3];
    bool ok = true;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        float p[3] = {g[0], g[1], g[2]}, q[3] = {g[0], g[1], g[2]};
        p[i] = g[i] + 1.0f;
        q[i] = g[i] - 1.0f;
        float Fp = 0.0f, Fq = 0.0f;
        ok = ok && ray_sample(V, wthr, p[0], p[1], p[2], Fp);
        ok = ok && ray_sample(V, wthr, q[0], q[1], q[2], Fq);
        n[i] = Fp - Fq;
    }
    m[0] = m[1] = m[2] = 0.0f;
    if (!ok) return false;
#pragma unroll
    for (int j = 0; j < 3; ++j) m[j] = (V.r[j] * n[0] + V.r[3 + j] * n[1]) + V.r[6 + j] * n[2];
    const float len = sqrtf((m[0] * m[0] + m[1] * m[1]) + m[2] * m[2]);
    if (!(__builtin_isfinite(len) && len > 0.0f)) {
        m[0] = m[1] = m[2] = 0.0f;
        return false;
    }
#pragma unroll
    for (int j = 0; j < 3; ++j) m[j] = m[j] / len;
    return true;
}

__device__ __forceinline__ int64_t ray_voxel(const RayVolume &V, const float g[3])
{
    int c[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        float x = floorf(g[i] + 0.5f);
        x = x < 0.0f ? 0.0f : x;
        x = x > V.hi[i] ? V.hi[i] : x;
        c[i] = (int)x;
    }
    return ((int64_t)c[2] * V.dim[1] + c[1]) * V.dim[0] + c[0];
}

// pixel of this lane: a wavefront = an 8 x 8 tile, a workgroup = 16 x 16 pixels
__device__ __forceinline__ void ray_pixel(int &u, int &v)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    u = blockIdx.x * 16 + (wave & 1) * 8 + (lane & 7);
    v = blockIdx.y * 16 + (wave >> 1) * 8 + (lane >> 3);
}

__global__ __launch_bounds__(256) void raycast_volume(RaycastParams p)
{
    int u, v;
    ray_pixel(u, v);
    if (u >= p.W || v >= p.H) return;
    const RayVolume &V = p.vol;
    const float dcx = ((float)u - p.cx) / p.fx, dcy = ((float)v - p.cy) / p.fy;
    const float r = 1.0f / sqrtf((dcx * dcx + dcy * dcy) + 1.0f);
    float gd[3], t_enter, t_exit, ts = 0.0f;
    bool hit = ray_setup(V, dcx, dcy, p.near_m, p.far_m, gd, t_enter, t_exit);
    hit = hit && ray_march(V, p.wthr, gd, r, t_enter, t_exit, &ts);
    const int64_t px = (int64_t)v * p.W + u;
    float g[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) g[i] = V.go[i] + ts * gd[i];
    if (p.depth) p.depth[px] = hit ? ts : 0.0f;
    if (p.normal) {
        float m[3] = {0.0f, 0.0f, 0.0f};
        if (hit) ray_normal(V, p.wthr, g, m);
        p.normal[3 * px] = m[0];
        p.normal[3 * px + 1] = m[1];
        p.normal[3 * px + 2] = m[2];
    }
    if (p.label_out || p.colour_out) {
        const int64_t vox = hit ? ray_voxel(V, g) : 0;
        if (p.label_out) p.label_out[px] = hit ? p.label[vox] : (uint16_t)0;
        if (p.colour_out) p.colour_out[px] = hit ? p.colour[vox] : 0u;
    }
}

// Every member of a batch into one image (one launch, members in index order per lane, box culling against the best hit).
__global__ __launch_bounds__(256) void raycast_batch(BatchRaycastParams p)
{
    int u, v;
    ray_pixel(u, v);
    if (u >= p.W || v >= p.H) return;
    const float dcx = ((float)u - p.cx) / p.fx, dcy = ((float)v - p.cy) / p.fy;
    const float r = 1.0f / sqrtf((dcx * dcx + dcy * dcy) + 1.0f);
    float best = 0.0f;
    int who = -1;
    for (int i = 0; i < p.n; ++i) {
        const RayVolume &V = p.members[i];
        float gd[3], t_enter, t_exit, ts;
        if (!ray_setup(V, dcx, dcy, p.near_m, p.far_m, gd, t_enter, t_exit)) continue;
        if (who >= 0 && !(t_enter < best)) continue;
        if (ray_march(V, p.wthr, gd, r, t_enter, t_exit, &ts) && (who < 0 || ts < best)) {
            best = ts;
            who = i;
        }
    }
    const int64_t px = (int64_t)v * p.W + u;
    if (p.depth) p.depth[px] = who >= 0 ? best : 0.0f;
    if (p.member) p.member[px] = who;
    if (p.normal) {
        float m[3] = {0.0f, 0.0f, 0.0f};
        if (who >= 0) {
            const RayVolume &V = p.members[who];
            float gd[3], te, tx, g[3];
            ray_setup(V, dcx, dcy, p.near_m, p.far_m, gd, te, tx);   // the same gd bits as in the march
#pragma unroll
            for (int i = 0; i < 3; ++i) g[i] = V.go[i] + best * gd[i];
            ray_normal(V, p.wthr, g, m);
        }
        p.normal[3 * px] = m[0];
        p.normal[3 * px + 1] = m[1];
        p.normal[3 * px + 2] = m[2];
    }
}

}  // namespace tsdfk
