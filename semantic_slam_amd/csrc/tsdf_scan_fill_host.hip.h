// tsdf_scan_fill_host.hip.h -- host side of the lidar gap fill (tsdf_scan_fill_*, tsdf_scan_project_filled,
// tsdf_integrate_range_filled, tsdf_integrate_scan_filled; tsdf_scan_fill.hip.h states the rule), included at the end of
// tsdf_capi.hip after the lidar host header, whose scanner, checks and staging it shares.
#pragma once

namespace {

int scan_fill_params_ok(const char *who, const tsdf_scan_fill_params *p)
{
    if (p->max_span_u < 0 || p->max_span_u > tsdfk::kFillMaxSpan || p->max_span_v < 0 || p->max_span_v > tsdfk::kFillMaxSpan)
        return fail(TSDF_ERR_INVALID, "%s: max_span_u = %d, max_span_v = %d: both must lie in [0, %d]", who, p->max_span_u, p->max_span_v,
                    tsdfk::kFillMaxSpan);
    if (!std::isfinite(p->jump_rel) || !(p->jump_rel >= 0.0f))
        return fail(TSDF_ERR_INVALID, "%s: jump_rel must be finite and >= 0", who);
    return TSDF_OK;
}

inline dim3 scan_fill_grid(int H, int W)
{
    return dim3((unsigned)((W + tsdfk::kFillTileW - 1) / tsdfk::kFillTileW), (unsigned)((H + tsdfk::kFillTileH - 1) / tsdfk::kFillTileH));
}
inline size_t scan_fill_tiles(int H, int W)
{
    const dim3 g = scan_fill_grid(H, W);
    return (size_t)g.x * g.y;
}

// depth_dev -> filled_dev (different buffers), the kinds and the tiles' counts where asked for, queued on `st`.
int scan_fill_launch(const tsdf_scan_fill_params &p, int H, int W, const float *depth_dev, float *filled_dev, uint8_t *kind_dev,
                     uint32_t *counts_dev, hipStream_t st)
{
    tsdfk::ScanFill f;
    f.H = H; f.W = W; f.span_u = p.max_span_u; f.span_v = p.max_span_v; f.jump_rel = p.jump_rel;
    hipLaunchKernelGGL(tsdfk::scan_fill, scan_fill_grid(H, W), dim3(256), 0, st, f, depth_dev, filled_dev, kind_dev, counts_dev);
    HIP_TRY(hipGetLastError());
    return TSDF_OK;
}

// The scanner's fill block, at the first call that fills: filled image | one count per tile | kind image, in HBM and pinned.
struct ScanFillBlock {
    float *filled;
    uint32_t *counts;
    uint8_t *kind;
};
ScanFillBlock scan_fill_block(char *base, size_t n_px, size_t n_tiles)
{
    ScanFillBlock b;
    b.filled = reinterpret_cast<float *>(base);
    b.counts = reinterpret_cast<uint32_t *>(b.filled + n_px);
    b.kind = reinterpret_cast<uint8_t *>(b.counts + n_tiles);
    return b;
}

int scanner_fill_ensure(tsdf_scanner *s)
{
    int rc = scanner_ensure(s);
    if (rc || s->d_fill) return rc;
    const size_t n_px = (size_t)s->H * s->W, bytes = n_px * sizeof(float) + scan_fill_tiles(s->H, s->W) * sizeof(uint32_t) + n_px;
    DevPtr<char> d_fill;
    HostPtr<char> h_fill;
    HIP_TRY(dev_alloc(d_fill, bytes));
    HIP_TRY(host_alloc(h_fill, bytes, hipHostMallocDefault));
    s->d_fill = std::move(d_fill); s->h_fill = std::move(h_fill);
    return TSDF_OK;
}

// The scanner's depth image in HBM (the second of d_images) through the fill, and what was asked for onto the host.
int scanner_fill_and_fetch(tsdf_scanner *s, const tsdf_scan_fill_params &p, float *filled_host, uint8_t *kind_host, int64_t *n_filled)
{
    const size_t n_px = (size_t)s->H * s->W, n_tiles = scan_fill_tiles(s->H, s->W);
    const ScanFillBlock d = scan_fill_block(s->d_fill.get(), n_px, n_tiles), h = scan_fill_block(s->h_fill.get(), n_px, n_tiles);
    int rc = scan_fill_launch(p, s->H, s->W, s->d_images.get() + n_px, d.filled, kind_host ? d.kind : nullptr, n_filled ? d.counts : nullptr,
                              s->stream);
    if (rc) return rc;
    if (filled_host) HIP_TRY(hipMemcpyAsync(h.filled, d.filled, n_px * sizeof(float), hipMemcpyDeviceToHost, s->stream));
    if (kind_host) HIP_TRY(hipMemcpyAsync(h.kind, d.kind, n_px, hipMemcpyDeviceToHost, s->stream));
    if (n_filled) HIP_TRY(hipMemcpyAsync(h.counts, d.counts, n_tiles * sizeof(uint32_t), hipMemcpyDeviceToHost, s->stream));
    HIP_TRY(hipStreamSynchronize(s->stream));
    if (filled_host) std::memcpy(filled_host, h.filled, n_px * sizeof(float));
    if (kind_host) std::memcpy(kind_host, h.kind, n_px);
    if (n_filled) {
        int64_t total = 0;
        for (size_t t = 0; t < n_tiles; ++t) total += h.counts[t];
        *n_filled = total;
    }
    return TSDF_OK;
}

}  // namespace

extern "C" {

int tsdf_scan_fill_params_default(tsdf_scan_fill_params *out)
{
    if (!out) return fail(TSDF_ERR_INVALID, "tsdf_scan_fill_params_default: NULL argument");
    out->max_span_u = 5;      // the horizontal gaps of a 64-beam scan in a 1242 x 375 image are 2 ... 5 pixels,
    out->max_span_v = 8;      // the vertical ones 5 ... 8: one beam spacing is closed, two are not
    out->jump_rel = 0.05f;
    return TSDF_OK;
}

int tsdf_scan_fill_depth(tsdf_scanner *s, const tsdf_scan_fill_params *params, const float *depth_host, float *filled_host,
                         uint8_t *kind_host, int64_t *n_filled)
{
    const char *who = "tsdf_scan_fill_depth";
    if (!s || !params || !depth_host) return fail(TSDF_ERR_INVALID, "%s: NULL argument", who);
    if (!filled_host && !kind_host && !n_filled) return fail(TSDF_ERR_INVALID, "%s: NULL argument (all three outputs)", who);
    int rc = scan_fill_params_ok(who, params);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(s->device));
    rc = scanner_fill_ensure(s);
    if (rc) return rc;
    const size_t n_px = (size_t)s->H * s->W, img = n_px * sizeof(float);
    float *d_depth = s->d_images.get() + n_px, *h_depth = s->h_images.get() + n_px;
    tsdf_host::copy_to_pinned(h_depth, depth_host, img);      // (staged: filled_host may be depth_host)
    HIP_TRY(hipMemcpyAsync(d_depth, h_depth, img, hipMemcpyHostToDevice, s->stream));
    return scanner_fill_and_fetch(s, *params, filled_host, kind_host, n_filled);
}

int tsdf_scan_project_filled(tsdf_scanner *s, const float velo2img[12], const float cam_K[9], const tsdf_scan_fill_params *params,
                             const float *points_host, int64_t n_points, float *depth_host, uint8_t *kind_host, int64_t *n_filled)
{
    const char *who = "tsdf_scan_project_filled";
    if (!s || !velo2img || !cam_K || !params) return fail(TSDF_ERR_INVALID, "%s: NULL argument", who);
    if (!depth_host && !kind_host && !n_filled) return fail(TSDF_ERR_INVALID, "%s: NULL argument (all three outputs)", who);
    int rc = scan_points_ok(who, points_host, n_points);
    if (rc == TSDF_OK) rc = scan_matrix_ok(who, "velo2img", velo2img, 12);
    if (rc == TSDF_OK) rc = scan_camera_ok(who, cam_K);
    if (rc == TSDF_OK) rc = scan_fill_params_ok(who, params);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(s->device));
    rc = scanner_fill_ensure(s);
    if (rc) return rc;
    // points -> keys -> the sparse depth image -> the filled one, all in HBM
    rc = scan_splat_points(s->stage, velo2img, s->H, s->W, points_host, n_points, s->stream);
    if (rc) return rc;
    rc = scan_resolve_keys(s->stage, scan_camera(cam_K), s->H, s->W, nullptr, s->d_images.get() + (size_t)s->H * s->W, nullptr, s->stream);
    if (rc) return rc;
    return scanner_fill_and_fetch(s, *params, depth_host, kind_host, n_filled);
}

int tsdf_integrate_range_filled(tsdf_volume *v, const tsdf_scan_fill_params *params, const float *range_host, const float cam2world[16])
{
    const char *who = "tsdf_integrate_range_filled";
    if (!v || !params || !range_host || !cam2world) return fail(TSDF_ERR_INVALID, "%s: NULL argument", who);
    int rc = scan_volume_ok(who, v);
    if (rc == TSDF_OK) rc = scan_fill_params_ok(who, params);
    if (rc) return rc;
    const bool defer = v->defer_n > 1;
    rc = bind_device(v, !defer);
    if (rc) return rc;
    // as tsdf_integrate_range, with one more slot between the ranges and the frame: ranges -> sparse depth -> filled depth
    const int H = v->cfg.im_height, W = v->cfg.im_width;
    const size_t img = (size_t)H * W * sizeof(float);
    StoreSlot raw, sparse, frame;
    rc = stage_frame(v, img, [&](float *pinned) { tsdf_host::copy_to_pinned(pinned, range_host, img); }, raw);
    if (rc == TSDF_OK) rc = sparse.take(v, &v->store->frames, v->copy_stream);
    if (rc == TSDF_OK) rc = frame.take(v, &v->store->frames, v->copy_stream);
    if (rc) return rc;
    hipLaunchKernelGGL(tsdfk::scan_range_to_depth, dim3(scan_blocks((int64_t)H * W)), dim3(256), 0, v->copy_stream,
                       scan_camera(v->cfg.cam_K), H, W, raw.as<float>(), sparse.as<float>());
    HIP_TRY(hipGetLastError());
    rc = scan_fill_launch(*params, H, W, sparse.as<float>(), frame.as<float>(), nullptr, nullptr, v->copy_stream);
    if (rc) return rc;
    HIP_TRY(hipEventRecord(v->pend_copied, v->copy_stream));
    raw.release_after(&v->pend_copied);
    sparse.release_after(&v->pend_copied);
    return apply_host_frame(v, frame, cam2world, defer, true);
}

int tsdf_integrate_scan_filled(tsdf_volume *v, const float velo2img[12], const tsdf_scan_fill_params *params, const float *points_host,
                               int64_t n_points, const float cam2world[16])
{
    const char *who = "tsdf_integrate_scan_filled";
    if (!v || !velo2img || !params || !cam2world) return fail(TSDF_ERR_INVALID, "%s: NULL argument", who);
    int rc = scan_points_ok(who, points_host, n_points);
    if (rc == TSDF_OK) rc = scan_matrix_ok(who, "velo2img", velo2img, 12);
    if (rc == TSDF_OK) rc = scan_volume_ok(who, v);
    if (rc == TSDF_OK) rc = scan_fill_params_ok(who, params);
    if (rc) return rc;
    const bool defer = v->defer_n > 1;
    rc = bind_device(v, !defer);
    if (rc) return rc;
    // as tsdf_integrate_scan, resolved into a slot of its own and filled from there into the frame's
    const int H = v->cfg.im_height, W = v->cfg.im_width;
    rc = scan_splat_points(v->scan, velo2img, H, W, points_host, n_points, v->copy_stream);
    if (rc) return rc;
    StoreSlot sparse, frame;
    rc = sparse.take(v, &v->store->frames, v->copy_stream);
    if (rc == TSDF_OK) rc = frame.take(v, &v->store->frames, v->copy_stream);
    if (rc) return rc;
    rc = scan_resolve_keys(v->scan, scan_camera(v->cfg.cam_K), H, W, nullptr, sparse.as<float>(), nullptr, v->copy_stream);
    if (rc == TSDF_OK) rc = scan_fill_launch(*params, H, W, sparse.as<float>(), frame.as<float>(), nullptr, nullptr, v->copy_stream);
    if (rc) return rc;
    HIP_TRY(hipEventRecord(v->pend_copied, v->copy_stream));
    sparse.release_after(&v->pend_copied);
    return apply_host_frame(v, frame, cam2world, defer, true);
}

}  // extern "C"
