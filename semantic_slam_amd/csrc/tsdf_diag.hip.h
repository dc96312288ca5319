// tsdf_diag.hip.h -- host side of include/tsdf_hip_diag.h: timers, probes, device self-tests, statistics and tuning knobs.
//
// Included at the end of tsdf_capi.hip (it reads the handles' internals: streams, counters, brick shape, variant).  The
// kernels the self-tests and probes launch stay beside the product's (tsdf_kernels.hip.h, tsdf_multiframe.hip.h).
#pragma once

namespace {

// Device milliseconds between two HIP events recorded on the handle's stream around the work queue() puts there.  The
// closing event is recorded and waited for whatever queue() returned; a failure of queue() is the one reported.
template <typename Queue>
int time_on_stream(tsdf_volume *v, const char *who, float *elapsed_ms, Queue &&queue)
{
    Event e0, e1;
    HIP_TRY(event_create(e0, hipEventDefault));
    HIP_TRY(event_create(e1, hipEventDefault));
    HIP_TRY(hipEventRecord(e0, v->stream));
    const int rc = queue();
    hipError_t er = hipEventRecord(e1, v->stream);
    hipError_t es = hipEventSynchronize(e1);
    float ms = 0.f;
    hipError_t et = hipEventElapsedTime(&ms, e0, e1);
    if (rc) return rc;
    if (er != hipSuccess || es != hipSuccess || et != hipSuccess)
        return fail(TSDF_ERR_HIP, "%s: event timing failed", who);
    *elapsed_ms = ms;
    return TSDF_OK;
}

int frames_timed(tsdf_volume *v, const float *const *depth_dev, const uint8_t *const *masks_dev,
                 const float *cam2world, int32_t n_frames, float *elapsed_ms, const char *who)
{
    int rc = bind_device(v);
    if (rc) return rc;
    return time_on_stream(v, who, elapsed_ms, [&]() -> int { return integrate_frames(v, depth_dev, masks_dev, cam2world, n_frames); });
}

}  // namespace

extern "C" {

// ---- timers ----------------------------------------------------------------------------------------------------------

int tsdf_integrate_sequence_timed(tsdf_volume *v, const float *depth_dev, const float *cam2world,
                                  int32_t n_frames, float *elapsed_ms)
{
    if (!v || !depth_dev || !cam2world || n_frames <= 0 || !elapsed_ms)
        return fail(TSDF_ERR_INVALID, "tsdf_integrate_sequence_timed: bad argument");
    std::vector<const float *> depths((size_t)n_frames, depth_dev);
    return frames_timed(v, depths.data(), nullptr, cam2world, n_frames, elapsed_ms, "tsdf_integrate_sequence_timed");
}

int tsdf_integrate_frames_timed(tsdf_volume *v, const float *const *depth_dev, const uint8_t *const *masks_dev,
                                const float *cam2world, int32_t n_frames, float *elapsed_ms)
{
    if (!v || !depth_dev || !cam2world || n_frames <= 0 || !elapsed_ms)
        return fail(TSDF_ERR_INVALID, "tsdf_integrate_frames_timed: bad argument");
    for (int k = 0; k < n_frames; ++k)
        if (!depth_dev[k]) return fail(TSDF_ERR_INVALID, "tsdf_integrate_frames_timed: depth_dev[%d] is NULL", k);
    return frames_timed(v, depth_dev, masks_dev, cam2world, n_frames, elapsed_ms, "tsdf_integrate_frames_timed");
}

// ---- probes ----------------------------------------------------------------------------------------------------------

// Measurement aid ("hipGraph"): the same n one-frame launches queued call by call and replayed from a
// captured hipGraph, `iters` times each; device milliseconds per repetition by HIP events.  The volume ends up with
// 2 * iters * n more frames applied than before (both forms run).
int tsdf_probe_graph_replay(tsdf_volume *v, const float *depth_dev, const float *cam2world, int32_t n_frames, int32_t iters,
                            float *ms_launches, float *ms_graph)
{
    if (!v || !depth_dev || !cam2world || n_frames <= 0 || iters <= 0 || !ms_launches || !ms_graph)
        return fail(TSDF_ERR_INVALID, "tsdf_probe_graph_replay: bad argument");
    int rc = bind_device(v);
    if (rc) return rc;
    std::vector<float> c2b((size_t)n_frames * 16);
    for (int k = 0; k < n_frames; ++k) compose_cam2base(v, cam2world + 16 * k, c2b.data() + 16 * k);
    auto queue_all = [&]() -> int {
        for (int k = 0; k < n_frames; ++k) {
            int r = launch_integrate(v, depth_dev, nullptr, c2b.data() + 16 * k);
            if (r) return r;
        }
        return TSDF_OK;
    };
    rc = queue_all();                                   // warm-up (and the summary's one-off work)
    if (rc) return rc;
    rc = time_on_stream(v, "tsdf_probe_graph_replay", ms_launches, [&]() -> int {
        int r = TSDF_OK;
        for (int i = 0; i < iters && r == TSDF_OK; ++i) r = queue_all();
        return r;
    });
    if (rc) return rc;
    *ms_launches /= (float)iters;
    Graph graph;
    GraphExec exec;
    HIP_TRY(hipStreamBeginCapture(v->stream, hipStreamCaptureModeThreadLocal));
    rc = queue_all();
    hipError_t ce = hipStreamEndCapture(v->stream, graph.put());
    if (rc) return rc;
    if (ce != hipSuccess) return fail(TSDF_ERR_HIP, "tsdf_probe_graph_replay: capture failed: %s", hipGetErrorString(ce));
    HIP_TRY(hipGraphInstantiate(exec.put(), graph, nullptr, nullptr, 0));
    HIP_TRY(hipGraphLaunch(exec, v->stream));           // warm-up
    rc = time_on_stream(v, "tsdf_probe_graph_replay", ms_graph, [&]() -> int {
        for (int i = 0; i < iters; ++i) HIP_TRY(hipGraphLaunch(exec, v->stream));
        return TSDF_OK;
    });
    if (rc) return rc;
    *ms_graph /= (float)iters;
    return TSDF_OK;
}

int tsdf_probe_stream(tsdf_volume *v, int32_t non_temporal, int32_t n_iters, float *elapsed_ms)
{
    if (!v || n_iters <= 0 || !elapsed_ms) return fail(TSDF_ERR_INVALID, "tsdf_probe_stream: bad argument");
    int rc = bind_device(v);
    if (rc) return rc;
    if (v->geo.n_vox % 4 != 0 || v->geo.n_vox == 0) return fail(TSDF_ERR_INVALID, "tsdf_probe_stream: slab voxels must be a positive multiple of 4");
    const size_t nq = (size_t)v->geo.n_vox / 4;
    const int blocks = (int)std::min<size_t>((nq + 255) / 256, (size_t)256 * 8);
    return time_on_stream(v, "tsdf_probe_stream", elapsed_ms, [&]() -> int {
        for (int i = 0; i < n_iters; ++i) {
            if (non_temporal) hipLaunchKernelGGL(tsdfk::stream_rmw<true>, dim3(blocks), dim3(256), 0, v->stream, v->d_tsdf, v->d_weight, nq, 1.0f, 0.0f);
            else hipLaunchKernelGGL(tsdfk::stream_rmw<false>, dim3(blocks), dim3(256), 0, v->stream, v->d_tsdf, v->d_weight, nq, 1.0f, 0.0f);
        }
        return TSDF_OK;
    });
}

// ---- device self-tests -----------------------------------------------------------------------------------------------

int tsdf_selftest_fastdiv(int32_t device, uint64_t seed, uint64_t n_samples, float fx, float cx,
                          uint64_t *mismatches, float first_bad[4])
{
    if (!mismatches || !first_bad) return fail(TSDF_ERR_INVALID, "tsdf_selftest_fastdiv: NULL argument");
    HIP_TRY(hipSetDevice(device));
    DevPtr<unsigned long long> d_cnt;
    DevPtr<float> d_bad;
    HIP_TRY(dev_alloc(d_cnt, sizeof(unsigned long long)));
    HIP_TRY(dev_alloc(d_bad, 4 * sizeof(float)));
    HIP_TRY(hipMemset(d_cnt, 0, sizeof(unsigned long long)));
    HIP_TRY(hipMemset(d_bad, 0, 4 * sizeof(float)));
    hipLaunchKernelGGL(tsdfk::selftest_fastdiv, dim3(256 * 8), dim3(256), 0, 0, seed, n_samples, fx, cx, d_cnt, d_bad);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipDeviceSynchronize();
    unsigned long long cnt = 0;
    if (e == hipSuccess) e = hipMemcpy(&cnt, d_cnt, sizeof cnt, hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(first_bad, d_bad, 4 * sizeof(float), hipMemcpyDeviceToHost);
    if (e != hipSuccess) return fail(TSDF_ERR_HIP, "tsdf_selftest_fastdiv: %s", hipGetErrorString(e));
    *mismatches = cnt;
    return TSDF_OK;
}

int tsdf_selftest_fastdiv_band(int32_t device, uint64_t seed, uint64_t n_samples, uint64_t *mismatches, float first_bad[4])
{
    if (!mismatches || !first_bad) return fail(TSDF_ERR_INVALID, "tsdf_selftest_fastdiv_band: NULL argument");
    HIP_TRY(hipSetDevice(device));
    DevPtr<unsigned long long> d_cnt;
    DevPtr<float> d_bad;
    HIP_TRY(dev_alloc(d_cnt, sizeof(unsigned long long)));
    HIP_TRY(dev_alloc(d_bad, 4 * sizeof(float)));
    HIP_TRY(hipMemset(d_cnt, 0, sizeof(unsigned long long)));
    HIP_TRY(hipMemset(d_bad, 0, 4 * sizeof(float)));
    hipLaunchKernelGGL(tsdfk::selftest_fastdiv_band, dim3(256 * 8), dim3(256), 0, 0, seed, n_samples, d_cnt, d_bad);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipDeviceSynchronize();
    unsigned long long cnt = 0;
    if (e == hipSuccess) e = hipMemcpy(&cnt, d_cnt, sizeof cnt, hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(first_bad, d_bad, 4 * sizeof(float), hipMemcpyDeviceToHost);
    if (e != hipSuccess) return fail(TSDF_ERR_HIP, "tsdf_selftest_fastdiv_band: %s", hipGetErrorString(e));
    *mismatches = cnt;
    return TSDF_OK;
}

int tsdf_selftest_round(int32_t device, uint64_t *mismatches, float first_bad[4])
{
    if (!mismatches || !first_bad) return fail(TSDF_ERR_INVALID, "tsdf_selftest_round: NULL argument");
    HIP_TRY(hipSetDevice(device));
    DevPtr<unsigned long long> d_cnt;
    DevPtr<float> d_bad;
    HIP_TRY(dev_alloc(d_cnt, sizeof(unsigned long long)));
    HIP_TRY(dev_alloc(d_bad, 4 * sizeof(float)));
    HIP_TRY(hipMemset(d_cnt, 0, sizeof(unsigned long long)));
    HIP_TRY(hipMemset(d_bad, 0, 4 * sizeof(float)));
    hipLaunchKernelGGL(tsdfk::selftest_round, dim3(256 * 8), dim3(256), 0, 0, d_cnt, d_bad);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipDeviceSynchronize();
    unsigned long long cnt = 0;
    if (e == hipSuccess) e = hipMemcpy(&cnt, d_cnt, sizeof cnt, hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(first_bad, d_bad, 4 * sizeof(float), hipMemcpyDeviceToHost);
    if (e != hipSuccess) return fail(TSDF_ERR_HIP, "tsdf_selftest_round: %s", hipGetErrorString(e));
    *mismatches = cnt;
    return TSDF_OK;
}

int tsdf_selftest_tile_tables(int32_t device, const float *depth_dev, const uint8_t *mask_dev, int32_t im_height,
                              int32_t im_width, float max_depth, uint64_t *mismatches)
{
    if (!depth_dev || !mismatches || im_height <= 0 || im_width <= 0)
        return fail(TSDF_ERR_INVALID, "tsdf_selftest_tile_tables: bad argument");
    HIP_TRY(hipSetDevice(device));
    uint64_t bad = 0;
    for (const int tile : {16, 8}) {      // both tile sizes the library uses (tsdf_host::tile_edge)
        const int tw = tsdf_host::tiles_along(im_width, tile), th = tsdf_host::tiles_along(im_height, tile);
        if (!tiles_fit(tw, th)) continue;
        const size_t per = tsdf_host::tile_table_elems(tw, th);
        DevPtr<float2> d_a, d_b;
        HIP_TRY(dev_alloc(d_a, per * sizeof(float2)));
        if (dev_alloc(d_b, per * sizeof(float2)) != hipSuccess) return fail(TSDF_ERR_HIP, "tsdf_selftest_tile_tables: hipMalloc");
        (void)hipMemset(d_a, 0xff, per * sizeof(float2));
        (void)hipMemset(d_b, 0x7f, per * sizeof(float2));
        tsdfk::TileSummaryParams tp;
        for (int f = 0; f < tsdfk::kMaxFramesPerLaunch; ++f) { tp.depth[f] = depth_dev; tp.mask[f] = mask_dev; }
        tp.H = im_height; tp.W = im_width; tp.tiles_w = tw; tp.tiles_h = th; tp.max_depth = max_depth;
        const unsigned lj = (unsigned)tsdf_host::tile_levels(tw);
        // a: the kernels the library launches (strips of 64 pixels; doubling in LDS when the frame's tiles fit)
        tp.tiles = d_a;
        if (tile == 16)
            hipLaunchKernelGGL(tsdfk::depth_tile_summary<16>, to_dim3(tsdf_host::grid_tile_strips(tw, th, 16, 1)), dim3(64, 4), 0, 0, tp);
        else
            hipLaunchKernelGGL(tsdfk::depth_tile_summary<8>, to_dim3(tsdf_host::grid_tile_strips(tw, th, 8, 1)), dim3(64, 4), 0, 0, tp);
        if (tw * th <= tsdfk::kTileLdsEntries)
            hipLaunchKernelGGL(tsdfk::tile_sparse_table, dim3(lj, 1), dim3(tw * th > 2048 ? 1024 : 256), 0, 0, d_a, tw, th, (unsigned long long *)nullptr);
        else
            hipLaunchKernelGGL(tsdfk::tile_sparse_table_scan, dim3(lj, 1), dim3(256), 0, 0, d_a, tw, th);
        // b: one wavefront per tile, levels by scanning
        tp.tiles = d_b;
        if (tile == 16)
            hipLaunchKernelGGL(tsdfk::depth_tile_summary_per_tile<16>, dim3((unsigned)((tw * th + 3) / 4), 1), dim3(64, 4), 0, 0, tp);
        else
            hipLaunchKernelGGL(tsdfk::depth_tile_summary_per_tile<8>, dim3((unsigned)((tw * th + 3) / 4), 1), dim3(64, 4), 0, 0, tp);
        hipLaunchKernelGGL(tsdfk::tile_sparse_table_scan, dim3(lj, 1), dim3(256), 0, 0, d_b, tw, th);
        hipError_t e = hipGetLastError();
        if (e == hipSuccess) e = hipDeviceSynchronize();
        std::vector<float2> a(per), b(per);
        if (e == hipSuccess) e = hipMemcpy(a.data(), d_a, per * sizeof(float2), hipMemcpyDeviceToHost);
        if (e == hipSuccess) e = hipMemcpy(b.data(), d_b, per * sizeof(float2), hipMemcpyDeviceToHost);
        if (e != hipSuccess) return fail(TSDF_ERR_HIP, "tsdf_selftest_tile_tables: %s", hipGetErrorString(e));
        for (size_t i = 0; i < per; ++i) bad += std::memcmp(&a[i], &b[i], sizeof(float2)) != 0;
    }
    {   // the fine table (4-pixel tiles, nine levels): the two kernels the library launches against the pixel-by-pixel one
        const int fw = tsdf_host::tiles_along(im_width, tsdfk::kFineTile), fh = tsdf_host::tiles_along(im_height, tsdfk::kFineTile);
        const size_t per = tsdfk::fine_table_elems(fw, fh);
        DevPtr<float2> d_a, d_b;
        HIP_TRY(dev_alloc(d_a, per * sizeof(float2)));
        if (dev_alloc(d_b, per * sizeof(float2)) != hipSuccess) return fail(TSDF_ERR_HIP, "tsdf_selftest_tile_tables: hipMalloc");
        (void)hipMemset(d_a, 0xff, per * sizeof(float2));
        (void)hipMemset(d_b, 0x7f, per * sizeof(float2));
        tsdfk::FineTileParams fp;
        for (int f = 0; f < tsdfk::kMaxFramesPerLaunch; ++f) { fp.depth[f] = depth_dev; fp.mask[f] = mask_dev; }
        fp.H = im_height; fp.W = im_width; fp.fw = fw; fp.fh = fh; fp.max_depth = max_depth;
        // b: pixel by pixel
        fp.fine = d_b;
        hipLaunchKernelGGL(tsdfk::fine_table_reference, dim3((unsigned)((per + 255) / 256), 1), dim3(256), 0, 0, fp);
        hipError_t e = hipGetLastError();
        if (e == hipSuccess) e = hipDeviceSynchronize();
        std::vector<float2> a(per), b(per);
        if (e == hipSuccess) e = hipMemcpy(b.data(), d_b, per * sizeof(float2), hipMemcpyDeviceToHost);
        // a: the standalone kernels (base tiles, then levels), then what a launch runs -- level (0, 0) out of the 8-pixel strip
        // kernel's pass, the upper levels by the extra workgroups of the sparse-table kernel
        for (int how = 0; how < 2 && e == hipSuccess; ++how) {
            (void)hipMemset(d_a, 0xff, per * sizeof(float2));
            if (how == 0) {
                fp.fine = d_a;
                hipLaunchKernelGGL(tsdfk::fine_tile_base, dim3((unsigned)((fw + 63) / 64), (unsigned)fh, 1), dim3(64), 0, 0, fp);
                hipLaunchKernelGGL(tsdfk::fine_tile_levels, dim3((unsigned)((fw * fh + 255) / 256), 1), dim3(256), 0, 0, d_a, fw, fh);
            } else {
                const int tw = tsdf_host::tiles_along(im_width, 8), th = tsdf_host::tiles_along(im_height, 8);
                if ((int64_t)tw * th > tsdfk::kTileLdsEntries) break;
                DevPtr<float2> d_c;
                if (dev_alloc(d_c, tsdf_host::tile_table_elems(tw, th) * sizeof(float2)) != hipSuccess) { e = hipErrorOutOfMemory; break; }
                tsdfk::TileSummaryParams tp;
                for (int f = 0; f < tsdfk::kMaxFramesPerLaunch; ++f) { tp.depth[f] = depth_dev; tp.mask[f] = mask_dev; }
                tp.H = im_height; tp.W = im_width; tp.tiles_w = tw; tp.tiles_h = th; tp.max_depth = max_depth;
                tp.tiles = d_c; tp.fine = d_a; tp.fw = fw; tp.fh = fh;
                hipLaunchKernelGGL(tsdfk::depth_tile_summary<8>, to_dim3(tsdf_host::grid_tile_strips(tw, th, 8, 1)), dim3(64, 4), 0, 0, tp);
                const unsigned threads = tw * th > 2048 ? 1024 : 256;
                hipLaunchKernelGGL(tsdfk::tile_sparse_table, dim3((unsigned)tsdf_host::tile_levels(tw) + ((unsigned)(fw * fh) + threads - 1) / threads, 1), dim3(threads), 0, 0,
                                   d_c, tw, th, (unsigned long long *)nullptr, d_a, fw, fh);
                e = hipGetLastError();
                if (e == hipSuccess) e = hipDeviceSynchronize();
            }
            if (e == hipSuccess) e = hipGetLastError();
            if (e == hipSuccess) e = hipDeviceSynchronize();
            if (e == hipSuccess) e = hipMemcpy(a.data(), d_a, per * sizeof(float2), hipMemcpyDeviceToHost);
            if (e == hipSuccess) for (size_t i = 0; i < per; ++i) bad += std::memcmp(&a[i], &b[i], sizeof(float2)) != 0;
        }
        if (e != hipSuccess) return fail(TSDF_ERR_HIP, "tsdf_selftest_tile_tables (fine): %s", hipGetErrorString(e));
    }
    *mismatches = bad;
    return TSDF_OK;
}

// ---- statistics ------------------------------------------------------------------------------------------------------

int32_t tsdf_frames_per_launch(const tsdf_volume *v)
{
    if (!v) return 0;
    return can_fuse(v) ? frames_per_launch(v) : 1;
}

int tsdf_shortcut_stats(tsdf_volume *v, int32_t enable, uint64_t counts_out[3])
{
    if (!v) return fail(TSDF_ERR_INVALID, "tsdf_shortcut_stats: NULL handle");
    int rc = bind_device(v);
    if (rc) return rc;
    HIP_TRY(hipStreamSynchronize(v->stream));
    if (counts_out) {
        unsigned int h[3] = {0, 0, 0};
        if (v->d_shortcut_stats) HIP_TRY(hipMemcpy(h, v->d_shortcut_stats, sizeof h, hipMemcpyDeviceToHost));
        for (int i = 0; i < 3; ++i) counts_out[i] = h[i];
    }
    if (enable && !v->d_shortcut_stats) HIP_TRY(dev_alloc(v->d_shortcut_stats, 8 * sizeof(unsigned int)));
    if (v->d_shortcut_stats) {
        if (enable) HIP_TRY(hipMemset(v->d_shortcut_stats, 0, 8 * sizeof(unsigned int)));
        else v->d_shortcut_stats.reset();
    }
    return TSDF_OK;
}

int tsdf_brick_list_stats(tsdf_volume *v, uint64_t counts_out[4])
{
    if (!v || !counts_out) return fail(TSDF_ERR_INVALID, "tsdf_brick_list_stats: NULL argument");
    int rc = bind_device(v);
    if (rc) return rc;
    HIP_TRY(hipStreamSynchronize(v->stream));
    unsigned int h[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (v->d_shortcut_stats) HIP_TRY(hipMemcpy(h, v->d_shortcut_stats, sizeof h, hipMemcpyDeviceToHost));
    for (int i = 0; i < 4; ++i) counts_out[i] = h[3 + i];
    return TSDF_OK;
}

int tsdf_classification_info(tsdf_volume *v, double info_out[2])
{
    if (!v || !info_out) return fail(TSDF_ERR_INVALID, "tsdf_classification_info: NULL argument");
    int rc = bind_device(v);
    if (rc) return rc;
    HIP_TRY(hipStreamSynchronize(v->stream));
    if (v->rb_stream) HIP_TRY(hipStreamSynchronize(v->rb_stream));     // (a pipelined launch's counters travel on their own stream)
    if (v->claims_pending && hipEventQuery(v->claims_done) == hipSuccess) {
        v->claim_fraction = claims_read_back(v);
        v->claims_pending = false;
        v->claims_known = true;
    }
    info_out[0] = v->claims_known ? v->claim_fraction : -1.0;
    info_out[1] = (double)v->launches_unclassified;
    return TSDF_OK;
}

int tsdf_summary_stats(tsdf_volume *v, uint64_t out[3])
{
    if (!v || !out) return fail(TSDF_ERR_INVALID, "tsdf_summary_stats: NULL argument");
    int rc = bind_device(v);
    if (rc) return rc;
    out[0] = out[1] = out[2] = 0;
    if (v->geo.n_flags == 0) { HIP_TRY(hipStreamSynchronize(v->stream)); return TSDF_OK; }
    DevPtr<unsigned long long> d;
    HIP_TRY(dev_alloc(d, 3 * sizeof(unsigned long long)));
    HIP_TRY(hipMemsetAsync(d, 0, 3 * sizeof(unsigned long long), v->stream));
    hipLaunchKernelGGL(tsdfk::summary_stats, to_dim3(tsdf_host::grid_summary_words(v->geo)), dim3(256), 0, v->stream, (const uint32_t *)v->d_flags.get(),
                       v->geo.n_flags, d.get());
    HIP_TRY(hipGetLastError());
    unsigned long long h[3] = {0, 0, 0};
    HIP_TRY(hipMemcpyAsync(h, d, sizeof h, hipMemcpyDeviceToHost, v->stream));
    HIP_TRY(hipStreamSynchronize(v->stream));
    out[0] = v->geo.n_flags; out[1] = h[1]; out[2] = h[2];
    return TSDF_OK;
}

int tsdf_summary_words(tsdf_volume *v, uint32_t *out_host, int64_t capacity, int64_t *count)
{
    if (!v || !count || capacity < 0 || (capacity > 0 && !out_host)) return fail(TSDF_ERR_INVALID, "tsdf_summary_words: bad argument");
    int rc = bind_device(v);
    if (rc) return rc;
    *count = (int64_t)v->geo.n_flags;
    if (v->geo.n_flags > 0 && capacity >= (int64_t)v->geo.n_flags)
        HIP_TRY(hipMemcpyAsync(out_host, v->d_flags.get(), v->geo.n_flags * sizeof(uint32_t), hipMemcpyDeviceToHost, v->stream));
    HIP_TRY(hipStreamSynchronize(v->stream));
    return TSDF_OK;
}

// (under the store's mutex alone: binding would apply the collected frames, whose slots are what the caller wants to see)
int tsdf_store_stats(tsdf_volume *v, int64_t out[9])
{
    if (!v || !out) return fail(TSDF_ERR_INVALID, "tsdf_store_stats: NULL argument");
    tsdf_store::store_counts(v->store, v, out);
    return TSDF_OK;
}

int tsdf_last_cam2base(const tsdf_volume *v, float out[16])
{
    if (!v || !out) return fail(TSDF_ERR_INVALID, "tsdf_last_cam2base: NULL argument");
    std::memcpy(out, v->last_cam2base, sizeof v->last_cam2base);
    return TSDF_OK;
}

// ---- tuning knobs ----------------------------------------------------------------------------------------------------

int tsdf_set_kernel_variant(tsdf_volume *v, int32_t variant)
{
    if (!v) return fail(TSDF_ERR_INVALID, "tsdf_set_kernel_variant: NULL handle");
    if (!variant_of(variant).known)
        return fail(TSDF_ERR_INVALID, "tsdf_set_kernel_variant: unknown variant %d (this build knows 0, 1, 3, 7, 8%s)", variant,
                    kExperiments ? " and the experiments" : "; the others live in the -DTSDF_EXPERIMENTS build");
    v->variant = variant;
    return TSDF_OK;
}

int tsdf_set_brick_shape(tsdf_volume *v, int32_t quads, int32_t rows, int32_t slices)
{
    if (!v) return fail(TSDF_ERR_INVALID, "tsdf_set_brick_shape: NULL handle");
    if (quads == 0 && rows == 0 && slices == 0) { choose_brick(v); return TSDF_OK; }
    if (!brick_shape_ok(v->cfg, quads, rows, slices))
        return fail(TSDF_ERR_INVALID, "tsdf_set_brick_shape: %d quads x %d rows x %d slices: needs quads * rows * slices <= 64 and "
                    "quads dividing dim_x / 4 = %d", quads, rows, slices, v->cfg.dim_x / 4);
    set_brick(v, quads, rows, slices);
    return TSDF_OK;
}

int tsdf_brick_shape(const tsdf_volume *v, int32_t shape_out[3])
{
    if (!v || !shape_out) return fail(TSDF_ERR_INVALID, "tsdf_brick_shape: NULL argument");
    shape_out[0] = v->geo.brick_q; shape_out[1] = v->geo.brick_q ? v->geo.brick_r : 0; shape_out[2] = v->geo.brick_q ? v->geo.brick_s : 0;
    return TSDF_OK;
}

int tsdf_default_brick_shape(const tsdf_config *cfg, int32_t shape_out[3])
{
    if (!cfg || !shape_out) return fail(TSDF_ERR_INVALID, "tsdf_default_brick_shape: NULL argument");
    if (cfg->dim_x <= 0 || cfg->dim_y <= 0 || cfg->z_end < cfg->z_begin)
        return fail(TSDF_ERR_INVALID, "tsdf_default_brick_shape: bad grid");
    int q, r, s;
    choose_brick_for(*cfg, q, r, s);
    shape_out[0] = q; shape_out[1] = q ? r : 0; shape_out[2] = q ? s : 0;
    return TSDF_OK;
}

// ---- tables ------------------------------------------------------------------------------------------------------------

int tsdf_scan_ground_tables(const tsdf_scan_ground_params *params, float *ring_tan_out, float *col_cos_out, float *col_sin_out,
                            float slopes_out[2], int32_t quad_first_out[4], int32_t quad_len_out[4])
{
    const char *who = "tsdf_scan_ground_tables";
    if (!params || !ring_tan_out || !col_cos_out || !col_sin_out || !slopes_out || !quad_first_out || !quad_len_out)
        return fail(TSDF_ERR_INVALID, "%s: NULL argument", who);
    tsdf_host::ScanGroundTables t;
    const tsdf_host::GroundLimit l = tsdf_host::build_scan_ground_tables(*params, t);      // the builder the scanners use
    if (l != tsdf_host::GroundLimit::Ok) return fail(TSDF_ERR_INVALID, "%s: ground_params: %s", who, tsdf_host::ground_limit_text(l));
    std::memcpy(ring_tan_out, t.T.data(), t.T.size() * sizeof(float));
    std::memcpy(col_cos_out, t.C.data(), t.C.size() * sizeof(float));
    std::memcpy(col_sin_out, t.S.data(), t.S.size() * sizeof(float));
    slopes_out[0] = t.tlo; slopes_out[1] = t.thi;
    for (int q = 0; q < 4; ++q) { quad_first_out[q] = t.first[q]; quad_len_out[q] = t.len[q]; }
    return TSDF_OK;
}

}  // extern "C"
