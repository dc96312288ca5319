/*
 * tsdf_hip_diag.h -- measurement and tuning aids of libtsdf_hip.so.
 *
 * Benchmark timers, probes, device self-tests, statistics and tuning knobs, used by bench.py, tools/ and tests/.  They
 * live in the same libtsdf_hip.so as the calls of tsdf_hip.h and follow its conventions, but they are not part of the
 * drop-in contract: a program that replaces the reference's TSDF needs tsdf_hip.h alone.
 */
#ifndef TSDF_HIP_DIAG_H
#define TSDF_HIP_DIAG_H

#include "tsdf_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- timers ---- */

/*
 * Timing aid for benchmarks: queue n_frames integrations of one device-resident depth frame
 * with poses cam2world[k*16..] back to back on the handle's stream, bracketed by HIP events
 * on that stream; *elapsed_ms is the device time between the events.  Synchronous.
 */
int tsdf_integrate_sequence_timed(tsdf_volume *vol, const float *depth_dev, const float *cam2world,
                                  int32_t n_frames, float *elapsed_ms);

/*
 * The same for a sequence whose frames each bring their own depth image (and optional instance mask): exactly
 * tsdf_integrate_frames_device, bracketed by HIP events on the handle's stream.  Synchronous.
 */
int tsdf_integrate_frames_timed(tsdf_volume *vol, const float *const *depth_dev, const uint8_t *const *masks_dev,
                                const float *cam2world, int32_t n_frames, float *elapsed_ms);

/* ---- probes ---- */

/*
 * Measurement aid: n_frames one-frame launches (one resident depth frame, poses cam2world[k*16..]) queued call by call
 * against the same launches replayed from a captured hipGraph, iters repetitions each; device milliseconds per
 * repetition.  Applies 2 * iters * n_frames (+ warm-up) frames to the volume.  (small grids.)
 */
int tsdf_probe_graph_replay(tsdf_volume *vol, const float *depth_dev, const float *cam2world, int32_t n_frames,
                            int32_t iters, float *ms_launches, float *ms_graph);

/*
 * Ceiling probe: n_iters passes of a bare 16 B/voxel read-modify-write stream over the slab
 * (values unchanged), timed with HIP events.  non_temporal selects nt loads/stores.
 */
int tsdf_probe_stream(tsdf_volume *vol, int32_t non_temporal, int32_t n_iters, float *elapsed_ms);

/* ---- device self-tests ---- */

/*
 * Device self-test of the kernel's shared-reciprocal division against the compiler's IEEE
 * division on n_samples pseudo-random operand pairs in the range the kernel uses it for
 * (DESIGN.md section 4).  A quotient may differ from the IEEE one only below 2^-42 and only if the
 * pixel coordinate fl(fx*q + cx) it feeds is unchanged for the given fx, cx (any |fx| < 2^14 the
 * kernel's fast path admits).  *mismatches must come back 0; first_bad = {n, d, got, want} otherwise.
 */
int tsdf_selftest_fastdiv(int32_t device, uint64_t seed, uint64_t n_samples, float fx, float cx,
                          uint64_t *mismatches, float first_bad[4]);

/*
 * Device self-test of the truncated distance's division diff / trunc through the shared refined reciprocal (fused
 * kernels, csrc/tsdf_kernels.hip.h: fast_div_r) against the compiler's IEEE division on n_samples operand pairs drawn
 * from the domain the kernel admits: divisor in [2^-20, 2^20], numerator 0, NaN or of magnitude in [2^-81, 2^60].
 * Every quotient must be bit-identical.  *mismatches must come back 0; first_bad = {n, d, got, want} otherwise.
 */
int tsdf_selftest_fastdiv_band(int32_t device, uint64_t seed, uint64_t n_samples, uint64_t *mismatches,
                               float first_bad[4]);

/*
 * Exhaustive device self-test of the kernel's one-instruction pixel rounding (v_cvt_rpi_i32_f32)
 * against roundf for every fp32 value in (-0.5, 2^24].  *mismatches must come back 0;
 * first_bad = {u, got, want, 0} otherwise.
 */
int tsdf_selftest_round(int32_t device, uint64_t *mismatches, float first_bad[4]);

/*
 * Device self-test of the depth tile tables the classified launches consult: builds the table of one frame (depth x mask,
 * mask_dev may be NULL) with the kernels the library launches (whole-row strips, levels by doubling) and with the plain
 * ones (one wavefront per tile, levels by scanning), for both tile sizes the library uses (16 x 16 pixels; 8 x 8 for slabs of
 * 10 M voxels and more), and counts the entries that differ in any bit; *mismatches must come back 0.
 */
int tsdf_selftest_tile_tables(int32_t device, const float *depth_dev, const uint8_t *mask_dev, int32_t im_height,
                              int32_t im_width, float max_depth, uint64_t *mismatches);

/* ---- statistics ---- */

/* Frames tsdf_integrate_frames_device / tsdf_integrate_sequence_timed apply per pass over this slab (1 when
 * the selected kernel variant does not fuse frames). */
int32_t tsdf_frames_per_launch(const tsdf_volume *vol);
/*
 * Diagnostics of the fused path's per-wavefront patch classification (depth tile summaries): reads the
 * counters {wavefront-frames that took the per-voxel path, that were updated as free space without projecting
 * a voxel, that were skipped} accumulated since they were last enabled (counts_out may be NULL), then
 * enables (and zeroes) or disables them.  Off by default; synchronises the stream.
 */
int tsdf_shortcut_stats(tsdf_volume *vol, int32_t enable, uint64_t counts_out[3]);
/*
 * More of the same, for the classified fused launches' brick work list (csrc/tsdf_multiframe.hip.h, classify_brick_list),
 * accumulated while the counters of tsdf_shortcut_stats are enabled: {super-bricks every frame skipped, bricks put on the
 * work list, of those: bricks whose super-brick left frames undecided (they classify themselves), of those: bricks every
 * frame skipped after all}.  Synchronises the stream; does not reset.
 */
int tsdf_brick_list_stats(tsdf_volume *vol, uint64_t counts_out[4]);
/*
 * State of the per-launch decision whether to classify (default kernel variant): info_out[0] = fraction of the
 * workgroup-frames the last counted launch claimed (-1 before the first read-back), info_out[1] = launches that have
 * gone without classification since the last one that classified.  Synchronises the stream.
 */
int tsdf_classification_info(tsdf_volume *vol, double info_out[2]);

/*
 * The summary words of the slab (one per 256-voxel segment; csrc/host_derive.h, "the summary word"): out = {segments,
 * those whose word says that every TSDF value is 1 (bit 0), those whose word carries a weight run (bit 2: every weight
 * is the count in the word, and the one-frame kernel does not load them)}.  Applies the collected frames and synchronises
 * the stream; {0, 0, 0} for a grid without summary (dim_x % 4 != 0).
 */
int tsdf_summary_stats(tsdf_volume *vol, uint64_t out[3]);
/*
 * The summary words themselves, in the order the kernels index them (word of row segment s of row y of local slice z:
 * (z * dim_y + y) * (dim_x / 256) + s for rows of a multiple of 256 voxels; otherwise word of 256-voxel chunk c of slice z:
 * z * ceil(dim_x * dim_y / 256) + c).  *count = the number of words (0 for a grid without summary, dim_x % 4 != 0); they are
 * copied to out_host when capacity >= *count, and nothing is written to it otherwise (out_host may be NULL with capacity
 * 0 to ask for the count).  Read-only: applies the collected frames and synchronises the stream, as tsdf_summary_stats does.
 */
int tsdf_summary_words(tsdf_volume *vol, uint32_t *out_host, int64_t capacity, int64_t *count);

/*
 * The handle's share of the staging store that the handles of its device and image size have in common (frame, mask and
 * tile-table slots): for the frames, the masks and the tables in turn, out = {slots the handle holds, slots it has
 * released that no one has reused yet, slots the class has in the store}.  Reads the store's bookkeeping only: it applies no
 * collected frame and does not synchronise, so the frames a deferring handle has collected show as held.
 */
int tsdf_store_stats(tsdf_volume *vol, int64_t out[9]);

/* The relative pose used by the most recent integrate call (16 floats), for parity tests. */
int tsdf_last_cam2base(const tsdf_volume *vol, float out[16]);

/* ---- tuning knobs ---- */

/* Select the Integrate kernel variant (0 = default; others are listed in DESIGN.md). */
int tsdf_set_kernel_variant(tsdf_volume *vol, int32_t variant);

/*
 * Tuning knob (no reference counterpart; results never depend on it): the box of voxels one wavefront owns, and
 * classifies as a whole, in the classified launches (bricks): `quads` x 4 voxels of `rows` rows of `slices`
 * slices.  Needs quads * rows * slices <= 64 and quads dividing dim_x / 4; (0, 0, 0) returns to the library's choice
 * for the grid.  tsdf_brick_shape reads the shape in use ({0, 0, 0}: the grid has no brick view, dim_x % 4 != 0).
 */
int tsdf_set_brick_shape(tsdf_volume *vol, int32_t quads, int32_t rows, int32_t slices);
int tsdf_brick_shape(const tsdf_volume *vol, int32_t shape_out[3]);
/* The shape tsdf_create would choose for this grid (host arithmetic only: needs no device). */
int tsdf_default_brick_shape(const tsdf_config *cfg, int32_t shape_out[3]);

/* ---- tables ---- */

/*
 * The tables a scanner or a handle searches when it marks the ground of a scan under *params (csrc/scan_ground_tables.h; the
 * same builder, so the same bits): ring_tan_out n_rings + 1 floats, col_cos_out and col_sin_out n_columns floats each,
 * slopes_out = {tan(mount - tol), tan(mount + tol)}, and per quadrant of the (x, y) plane the first column of its run of
 * column boundaries and the run's length.  tests/scan_ground_spec.py takes them from here, so that it is held to the rule
 * and not to a second libm.  Host arithmetic only: needs no device.
 */
int tsdf_scan_ground_tables(const tsdf_scan_ground_params *params, float *ring_tan_out, float *col_cos_out,
                            float *col_sin_out, float slopes_out[2], int32_t quad_first_out[4],
                            int32_t quad_len_out[4]);

#ifdef __cplusplus
}
#endif
#endif /* TSDF_HIP_DIAG_H */
