// tsdf_segment_host.hip.h -- host side of geometric segmentation and mask refinement (tsdf_segment*; tsdf_segment.hip.h states the rule),
// included at the end of tsdf_capi.hip after the raycast and associate host headers, whose camera and mask-count checks it shares.
#pragma once

struct tsdf_segmenter {
    int device = 0, H = 0, W = 0;
    Stream own_stream;
    hipStream_t stream = nullptr;
    DevPtr<int4> d_pts;
    DevPtr<int32_t> d_parent, d_root, d_num, d_cluster, d_total;
    DevPtr<uint32_t> d_size, d_blocks;
    DevBuf<uint32_t> d_counts;                  // grown with C + C * K
    HostBuf<uint32_t> h_counts;
    HostPtr<int32_t> h_total;
};

namespace {

constexpr int64_t kSegMaxCountWords = (int64_t)1 << 24;   // C + C * K words of the refinement's count block

int seg_params_ok(const char *who, const tsdf_segment_params *p)
{
    if (!p) return fail(TSDF_ERR_INVALID, "%s: NULL parameters", who);
    int rc = camera_ok(who, p->cam_K, p->im_height, p->im_width, p->near_m, p->far_m);
    if (rc) return rc;
    if (p->far_m > 32.0f) return fail(TSDF_ERR_INVALID, "%s: far_m %g is above 32 m", who, (double)p->far_m);
    const struct { const char *name; float v; } radii[] = {{"small_radius_m", p->small_radius_m},
                                                            {"large_radius_m", p->large_radius_m},
                                                            {"seg_radius_m", p->seg_radius_m}};
    for (const auto &r : radii)
        if (!(std::isfinite(r.v) && r.v > 0.0f && r.v <= 32.0f))
            return fail(TSDF_ERR_INVALID, "%s: %s must be finite, > 0 and <= 32 m (%g)", who, r.name, (double)r.v);
    if (!(p->small_radius_m < p->large_radius_m))
        return fail(TSDF_ERR_INVALID, "%s: small_radius_m %g must be below large_radius_m %g", who, (double)p->small_radius_m,
                    (double)p->large_radius_m);
    if (!(std::isfinite(p->don_thresh) && p->don_thresh > 0.0f))
        return fail(TSDF_ERR_INVALID, "%s: don_thresh must be finite and > 0 (%g)", who, (double)p->don_thresh);
    if (p->min_cluster < 1) return fail(TSDF_ERR_INVALID, "%s: min_cluster %d is below 1", who, p->min_cluster);
    if (p->max_cluster < p->min_cluster)
        return fail(TSDF_ERR_INVALID, "%s: max_cluster %d is below min_cluster %d", who, p->max_cluster, p->min_cluster);
    if (!(p->overlap > 0.0f && p->overlap <= 1.0f))
        return fail(TSDF_ERR_INVALID, "%s: overlap must lie in (0, 1] (%g)", who, (double)p->overlap);
    if (p->inset < 0 || p->inset > tsdfk::kSegMaxInset)
        return fail(TSDF_ERR_INVALID, "%s: inset %d is outside 0..%d", who, p->inset, tsdfk::kSegMaxInset);
    return TSDF_OK;
}

int seg_handle_ok(const char *who, const tsdf_segmenter *s, const tsdf_segment_params *p)
{
    if (p->im_height != s->H || p->im_width != s->W)
        return fail(TSDF_ERR_INVALID, "%s: the parameters' image is %dx%d, the segmenter's %dx%d", who, p->im_width, p->im_height,
                    s->W, s->H);
    return TSDF_OK;
}

tsdfk::SegCamera seg_camera(const tsdf_segment_params *p)
{
    tsdfk::SegCamera k;
    k.fx = p->cam_K[0]; k.fy = p->cam_K[4]; k.cx = p->cam_K[2]; k.cy = p->cam_K[5];
    k.near_m = p->near_m; k.far_m = p->far_m; k.H = p->im_height; k.W = p->im_width;
    return k;
}

// DoN, labelling and numbering queued on the segmenter's stream; *n_clusters on the host when it returns.
int seg_depth(tsdf_segmenter *s, const tsdf_segment_params *p, const float *depth, float *don, int32_t *cluster,
                     int32_t *n_clusters)
{
    const int64_t n_px = (int64_t)s->H * s->W;
    const int nb = (int)((n_px + 255) / 256);
    const tsdfk::SegCamera k = seg_camera(p);
    hipStream_t st = s->stream;
    hipLaunchKernelGGL(tsdfk::seg_backproject, dim3(nb), dim3(256), 0, st, k, depth, s->d_pts.get());
    hipLaunchKernelGGL(tsdfk::seg_don, dim3((s->W + 15) / 16, (s->H + 15) / 16), dim3(256), 0, st, k, s->d_pts.get(),
                       p->small_radius_m, p->large_radius_m, p->don_thresh, don, s->d_parent.get());
    const int64_t Rs = (int64_t)std::rint(p->seg_radius_m * 8192.0f);
    hipLaunchKernelGGL(tsdfk::seg_merge, dim3(nb), dim3(256), 0, st, s->H, s->W, s->d_pts.get(), Rs * Rs, s->d_parent.get());
    HIP_TRY(hipMemsetAsync(s->d_size, 0, (size_t)n_px * sizeof(uint32_t), st));
    hipLaunchKernelGGL(tsdfk::seg_root_size, dim3(nb), dim3(256), 0, st, n_px, s->d_parent.get(), s->d_root.get(), s->d_size.get());
    const uint32_t lo = (uint32_t)p->min_cluster, hi = (uint32_t)p->max_cluster;
    hipLaunchKernelGGL(tsdfk::seg_block_count, dim3(nb), dim3(256), 0, st, n_px, s->d_root.get(), s->d_size.get(), lo, hi,
                       s->d_blocks.get());
    hipLaunchKernelGGL(tsdfk::seg_scan_blocks, dim3(1), dim3(1024), 0, st, s->d_blocks.get(), nb, s->d_total.get());
    hipLaunchKernelGGL(tsdfk::seg_number, dim3(nb), dim3(256), 0, st, n_px, s->d_root.get(), s->d_size.get(), lo, hi,
                       s->d_blocks.get(), s->d_num.get());
    hipLaunchKernelGGL(tsdfk::seg_label, dim3(nb), dim3(256), 0, st, n_px, s->d_root.get(), s->d_size.get(), lo, hi,
                       s->d_num.get(), cluster);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(s->h_total.get(), s->d_total.get(), sizeof(int32_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    *n_clusters = *s->h_total.get();
    return TSDF_OK;
}

int seg_refine(const char *who, tsdf_segmenter *s, const tsdf_segment_params *p, const int32_t *cluster, int32_t C,
                      const uint8_t *masks, int32_t K, uint8_t *out, uint32_t *counts_host)
{
    const int64_t n_px = (int64_t)s->H * s->W;
    const int64_t words = (int64_t)C + (int64_t)C * K;
    if (words > kSegMaxCountWords)
        return fail(TSDF_ERR_INVALID, "%s: %d clusters under %d masks need a count block of %lld words, above %lld", who, C, K,
                    (long long)words, (long long)kSegMaxCountWords);
    const size_t need = (size_t)std::max<int64_t>(words, 1);
    HIP_TRY(s->d_counts.ensure(need));
    if (counts_host) HIP_TRY(s->h_counts.ensure(need));
    hipStream_t st = s->stream;
    HIP_TRY(hipMemsetAsync(s->d_counts, 0, need * sizeof(uint32_t), st));
    tsdfk::SegRefine a;
    a.cluster = cluster; a.masks = masks; a.out = out; a.counts = s->d_counts;
    a.H = s->H; a.W = s->W; a.K = K; a.C = C; a.inset = p->inset; a.overlap = p->overlap;
    const dim3 grid((unsigned)((n_px + 255) / 256), (unsigned)K);
    hipLaunchKernelGGL(tsdfk::seg_refine_count, grid, dim3(256), 0, st, a);
    hipLaunchKernelGGL(tsdfk::seg_refine_accept, grid, dim3(256), 0, st, a);
    HIP_TRY(hipGetLastError());
    if (counts_host && words > 0)
        HIP_TRY(hipMemcpyAsync(s->h_counts.get(), s->d_counts.get(), (size_t)words * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (counts_host && words > 0) std::memcpy(counts_host, s->h_counts.get(), (size_t)words * sizeof(uint32_t));
    return TSDF_OK;
}

}  // namespace

extern "C" {

int tsdf_segment_params_default(const tsdf_config *cfg, tsdf_segment_params *out)
{
    if (!cfg || !out) return fail(TSDF_ERR_INVALID, "tsdf_segment_params_default: NULL argument");
    std::memcpy(out->cam_K, cfg->cam_K, sizeof out->cam_K);
    out->im_height = cfg->im_height;
    out->im_width = cfg->im_width;
    out->near_m = 0.0f;
    out->far_m = cfg->max_depth;
    out->small_radius_m = 0.05f;      // ref: config/TUM3.yaml:75
    out->large_radius_m = 0.5f;       // :76
    out->don_thresh = 0.1f;           // :77
    out->seg_radius_m = 0.05f;        // :78
    out->min_cluster = 15;            // ref: src/DoN.cpp:47
    out->max_cluster = 1000000;
    out->overlap = 0.5f;              // ref: config/TUM3.yaml:90
    out->inset = 2;                   // :85, mnDist = 1.0: more than one pixel inside the contour
    return TSDF_OK;
}

int tsdf_segmenter_destroy(tsdf_segmenter *s)
{
    if (!s) return TSDF_OK;
    (void)hipSetDevice(s->device);
    if (s->own_stream) (void)hipStreamSynchronize(s->own_stream);
    if (s->stream && s->stream != s->own_stream) (void)hipStreamSynchronize(s->stream);
    delete s;            // the owners release the memory and the stream (the device is current)
    return TSDF_OK;
}

int tsdf_segmenter_create(int32_t device, int32_t im_height, int32_t im_width, tsdf_segmenter **out)
{
    const char *who = "tsdf_segmenter_create";
    if (!out) return fail(TSDF_ERR_INVALID, "%s: NULL argument", who);
    *out = nullptr;
    int rc = image_ok(who, im_height, im_width);
    if (rc) return rc;
    int n_dev = 0;
    if (hipGetDeviceCount(&n_dev) != hipSuccess || n_dev <= 0)
        return fail(TSDF_ERR_NO_DEVICE, "%s: no HIP device visible (this library has no CPU path)", who);
    if (device < 0 || device >= n_dev) return fail(TSDF_ERR_INVALID, "%s: device %d not in [0,%d)", who, device, n_dev);
    tsdf_segmenter *s = new (std::nothrow) tsdf_segmenter();
    if (!s) return fail(TSDF_ERR_INVALID, "%s: out of host memory", who);
    s->device = device; s->H = im_height; s->W = im_width;
    auto cleanup = [&](int code) { tsdf_segmenter_destroy(s); return code; };
    HIP_TRY_OR(cleanup, hipSetDevice(device));
    HIP_TRY_OR(cleanup, stream_create(s->own_stream));
    s->stream = s->own_stream;
    const size_t n_px = (size_t)im_height * im_width, nb = (n_px + 255) / 256;
    HIP_TRY_OR(cleanup, dev_alloc(s->d_pts, n_px * sizeof(int4)));
    HIP_TRY_OR(cleanup, dev_alloc(s->d_parent, n_px * sizeof(int32_t)));
    HIP_TRY_OR(cleanup, dev_alloc(s->d_root, n_px * sizeof(int32_t)));
    HIP_TRY_OR(cleanup, dev_alloc(s->d_num, n_px * sizeof(int32_t)));
    HIP_TRY_OR(cleanup, dev_alloc(s->d_cluster, n_px * sizeof(int32_t)));
    HIP_TRY_OR(cleanup, dev_alloc(s->d_size, n_px * sizeof(uint32_t)));
    HIP_TRY_OR(cleanup, dev_alloc(s->d_blocks, nb * sizeof(uint32_t)));
    HIP_TRY_OR(cleanup, dev_alloc(s->d_total, sizeof(int32_t)));
    HIP_TRY_OR(cleanup, host_alloc(s->h_total, sizeof(int32_t), hipHostMallocDefault));
    *out = s;
    return TSDF_OK;
}

int tsdf_segmenter_set_stream(tsdf_segmenter *s, void *hip_stream)
{
    if (!s) return fail(TSDF_ERR_INVALID, "tsdf_segmenter_set_stream: NULL handle");
    HIP_TRY(hipSetDevice(s->device));
    HIP_TRY(hipStreamSynchronize(s->stream));  // do not reorder against work already queued
    s->stream = hip_stream ? (hipStream_t)hip_stream : s->own_stream.get();
    return TSDF_OK;
}

int tsdf_segment_depth_device(tsdf_segmenter *s, const tsdf_segment_params *p, const float *depth_dev, float *don_dev,
                              int32_t *cluster_dev, int32_t *n_clusters)
{
    const char *who = "tsdf_segment_depth_device";
    int rc = seg_params_ok(who, p);
    if (rc) return rc;
    if (!s || !depth_dev || !cluster_dev || !n_clusters) return fail(TSDF_ERR_INVALID, "%s: NULL argument", who);
    rc = seg_handle_ok(who, s, p);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(s->device));
    return seg_depth(s, p, depth_dev, don_dev, cluster_dev, n_clusters);
}

int tsdf_segment_refine_masks_device(tsdf_segmenter *s, const tsdf_segment_params *p, const int32_t *cluster_dev,
                                     int32_t n_clusters, const uint8_t *masks_dev, int32_t k, uint8_t *masks_out_dev,
                                     uint32_t *counts_host)
{
    const char *who = "tsdf_segment_refine_masks_device";
    int rc = seg_params_ok(who, p);
    if (rc == TSDF_OK) rc = masks_ok(who, k);
    if (rc) return rc;
    if (n_clusters < 0) return fail(TSDF_ERR_INVALID, "%s: n_clusters = %d is negative", who, n_clusters);
    if (!s || !cluster_dev || !masks_dev || !masks_out_dev) return fail(TSDF_ERR_INVALID, "%s: NULL argument", who);
    if (masks_out_dev == masks_dev) return fail(TSDF_ERR_INVALID, "%s: the masks cannot be refined in place", who);
    rc = seg_handle_ok(who, s, p);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(s->device));
    return seg_refine(who, s, p, cluster_dev, n_clusters, masks_dev, k, masks_out_dev, counts_host);
}

int tsdf_segment_frame(tsdf_segmenter *s, const tsdf_segment_params *p, const float *depth_dev, const uint8_t *masks_dev,
                       int32_t k, uint8_t *masks_out_dev, int32_t *cluster_dev, int32_t *n_clusters)
{
    const char *who = "tsdf_segment_frame";
    int rc = seg_params_ok(who, p);
    if (rc == TSDF_OK) rc = masks_ok(who, k);
    if (rc) return rc;
    if (!s || !depth_dev || !masks_dev || !masks_out_dev || !n_clusters) return fail(TSDF_ERR_INVALID, "%s: NULL argument", who);
    if (masks_out_dev == masks_dev) return fail(TSDF_ERR_INVALID, "%s: the masks cannot be refined in place", who);
    rc = seg_handle_ok(who, s, p);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(s->device));
    int32_t *cluster = cluster_dev ? cluster_dev : s->d_cluster.get();
    rc = seg_depth(s, p, depth_dev, nullptr, cluster, n_clusters);
    if (rc) return rc;
    return seg_refine(who, s, p, cluster, *n_clusters, masks_dev, k, masks_out_dev, nullptr);
}

}  // extern "C"
