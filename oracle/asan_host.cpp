// asan_host.cpp -- the product's HOST-side arithmetic (no device code) compiled for the CPU sanitizer run:
// semantic_slam_amd/csrc/pose_math.h (4x4 multiply / cofactor inverse, ref: src/tsdf.cu:253-403) and
// semantic_slam_amd/csrc/host_derive.h (wavefront brick choice, guards and margins of the exact shortcuts, launch policy, scratch block layout) and
// semantic_slam_amd/csrc/host_copy.h (the caller's frame into the pinned ring: streaming stores), behind plain C entry points, linked with tsdf_oracle.c into oracle/_asan/liboracle_asan.so by `make -C oracle asan`
// (-fsanitize=address,undefined -fno-sanitize-recover=all).  tests/test_sanitizers.py runs the golden vectors, the pose
// known-answer tests, the writers and these entry points under it.  TEST INFRASTRUCTURE: the headers are
// the product's own files, compiled here a second time; nothing in the product loads this library.
#include "../semantic_slam_amd/csrc/host_derive.h"
#include "../semantic_slam_amd/csrc/pose_math.h"
#include "../semantic_slam_amd/csrc/host_copy.h"

extern "C" {

void asan_multiply_matrix(const float *a, const float *b, float *out) { tsdf_host::multiply_matrix(a, b, out); }

int asan_invert_matrix(const float *m, float *out) { return tsdf_host::invert_matrix(m, out) ? 1 : 0; }

int asan_brick_shape_ok(const tsdf_config *c, int q, int r, int s) { return tsdf_host::brick_shape_ok(*c, q, r, s) ? 1 : 0; }

void asan_default_brick_shape(const tsdf_config *c, int32_t out[3])
{
    int q = 0, r = 0, s = 0;
    tsdf_host::choose_brick_default(*c, q, r, s);
    out[0] = q; out[1] = q ? r : 0; out[2] = q ? s : 0;     // as tsdf_default_brick_shape reports a grid without a brick view
}

// out: cz_margin, fast_ok, trunc_fast, cz_short, cz_pad, px_margin_u, px_margin_v
void asan_projection_guards(const tsdf_config *c, const float *cam2base, float out[7])
{
    const tsdf_host::ProjectionGuards g = tsdf_host::derive_projection_guards(*c, cam2base);
    out[0] = g.cz_margin; out[1] = (float)g.fast_ok; out[2] = (float)g.trunc_fast;
    out[3] = g.cz_short; out[4] = g.cz_pad; out[5] = g.px_margin_u; out[6] = g.px_margin_v;
}

// dst / src: any alignment, any size (the product hands it page-aligned ring slots and whole frames)
void asan_copy_to_pinned(void *dst, const void *src, size_t n) { tsdf_host::copy_to_pinned(dst, src, n); }

// ---- launch policy; mode: 0 adaptive, 1 never, 2 always (tsdf_host::Classify) ----
static tsdf_host::Classify mode_of(int mode) { return static_cast<tsdf_host::Classify>(mode); }

// out: fuses, scalar, classify mode; returns 1 for a shipped variant, else 0
int asan_decode_variant(int variant, int32_t out[3])
{
    const tsdf_host::Variant v = tsdf_host::decode_variant(variant);
    out[0] = v.fuses; out[1] = v.scalar; out[2] = static_cast<int32_t>(v.classify);
    return v.known ? 1 : 0;
}

int asan_tile_levels(int n) { return tsdf_host::tile_levels(n); }
int asan_tiles_fit(int tiles_w, int tiles_h) { return tsdf_host::tiles_fit(tiles_w, tiles_h) ? 1 : 0; }
int asan_tile_edge(const tsdf_config *c, int batch_member) { return tsdf_host::tile_edge(*c, batch_member != 0); }
int asan_fine_tables(const tsdf_config *c, int tile) { return tsdf_host::fine_tables(*c, tile) ? 1 : 0; }
size_t asan_launch_table_bytes(const tsdf_config *c, int tile, int fine) { return tsdf_host::launch_table_bytes(*c, tile, fine != 0); }
int asan_pipelines(const tsdf_config *c) { return tsdf_host::pipelines(*c) ? 1 : 0; }
int asan_classify_one_frame(int mode, int64_t launch_voxels) { return tsdf_host::classify_one_frame(mode_of(mode), launch_voxels) ? 1 : 0; }

int asan_classify_fused(int mode, int claims_known, double claim_fraction, int launches_unclassified)
{
    return tsdf_host::classify_fused(mode_of(mode), claims_known != 0, claim_fraction, launches_unclassified) ? 1 : 0;
}

// out: cache_lo, cache_hi
void asan_sweep_window(int nz, int dim_x, int dim_y, int64_t window_bytes, int reverse, int32_t out[2])
{
    const tsdf_host::SweepWindow w = tsdf_host::sweep_window(nz, dim_x, dim_y, window_bytes, reverse != 0);
    out[0] = w.cache_lo; out[1] = w.cache_hi;
}

int asan_batch_defers(int members, int64_t total_voxels) { return tsdf_host::batch_defers(members, total_voxels) ? 1 : 0; }
int asan_batch_classifies(int mode, int members, int64_t launch_voxels)
{
    return tsdf_host::batch_classifies(mode_of(mode), members, launch_voxels) ? 1 : 0;
}
int asan_batch_lanes(int members) { return tsdf_host::batch_lanes(members); }

// ---- scratch blocks: offsets[i] of n regions of bytes[i] carved in turn out of one block; returns the block's size ----
size_t asan_regions(const size_t *bytes, int n, size_t *offsets)
{
    tsdf_host::Regions r;
    for (int i = 0; i < n; ++i) offsets[i] = r.add(bytes[i]);
    return r.total();
}

}  // extern "C"
