// tsdf_scan_host.hip.h -- host side of the lidar path (tsdf_scan_*, tsdf_scanner_*, tsdf_integrate_range, tsdf_integrate_scan;
// tsdf_scan.hip.h states the rule), included at the end of tsdf_capi.hip after the raycast host header, whose image check it
// shares.
#pragma once

// A small object like tsdf_segmenter: scans of one image size on one device, on a stream of its own.  Nothing is allocated
// until the first call that needs it.
struct tsdf_scanner {
    int device = 0, H = 0, W = 0;
    Stream stream;
    ScanStage stage;
    DevPtr<float> d_images;          // range | depth
    DevPtr<uint32_t> d_counts;       // written pixels per workgroup of scan_resolve
    HostPtr<float> h_images;         // the pinned mirror of d_images, and behind it of d_counts
    DevPtr<char> d_fill;             // the gap fill's (tsdf_scan_fill_host.hip.h, at the first call that fills): filled depth |
    HostPtr<char> h_fill;            // one count per tile | kind; and its pinned mirror
    ScanGroundStage ground;          // the ground marking's (tsdf_scan_ground_host.hip.h, at the first call that marks)
};

namespace {

inline unsigned scan_blocks(int64_t n) { return (unsigned)((n + 255) / 256); }

int scan_matrix_ok(const char *who, const char *name, const float *m, int n)
{
    for (int i = 0; i < n; ++i)
        if (!std::isfinite(m[i])) return fail(TSDF_ERR_INVALID, "%s: %s[%d] is not finite", who, name, i);
    return TSDF_OK;
}

int scan_camera_ok(const char *who, const float cam_K[9])
{
    int rc = scan_matrix_ok(who, "cam_K", cam_K, 9);
    if (rc) return rc;
    if (cam_K[0] == 0.0f || cam_K[4] == 0.0f) return fail(TSDF_ERR_INVALID, "%s: fx and fy must be non-zero", who);
    return TSDF_OK;
}

int scan_points_ok(const char *who, const float *points_host, int64_t n_points)
{
    if (n_points < 0 || n_points > tsdfk::kScanMaxPoints)
        return fail(TSDF_ERR_INVALID, "%s: n_points = %lld is outside [0, %lld] (a point's index + 1 is the upper word of its pixel key)",
                    who, (long long)n_points, (long long)tsdfk::kScanMaxPoints);
    if (n_points > 0 && !points_host) return fail(TSDF_ERR_INVALID, "%s: NULL argument", who);
    return TSDF_OK;
}

tsdfk::ScanCamera scan_camera(const float cam_K[9])
{
    tsdfk::ScanCamera k;
    k.fx = cam_K[0]; k.fy = cam_K[4]; k.cx = cam_K[2]; k.cy = cam_K[5];
    return k;
}

// The scan's points into HBM and their keys into the key image, all queued on `st`; the caller's buffer is free when this
// returns.  n_points == 0 queues nothing but the key image's first clear.
// The three steps of it, which the ground marking (tsdf_scan_ground_host.hip.h) takes one by one with its own kernels in
// between: the key image there and all zero; the last scan's work over; the points in HBM.
int scan_keys_ready(ScanStage &s, size_t n_px, hipStream_t st)
{
    if (!s.pts_read) HIP_TRY(event_create(s.pts_read));
    if (!s.d_keys.fits(n_px)) { HIP_TRY(s.d_keys.ensure(n_px)); s.keys_clean = false; }
    if (!s.keys_clean) HIP_TRY(hipMemsetAsync(s.d_keys, 0, n_px * sizeof(unsigned long long), st));
    s.keys_clean = true;
    return TSDF_OK;
}
int scan_points_free(ScanStage &s)
{
    if (!s.pts_read) HIP_TRY(event_create(s.pts_read));
    if (s.pts_in_use) HIP_TRY(hipEventSynchronize(s.pts_read));   // the last scan's copy and kernels have run: both blocks are free
    s.pts_in_use = false;
    return TSDF_OK;
}
int scan_upload_points(ScanStage &s, const float *points_host, int64_t n_points, hipStream_t st)
{
    int rc = scan_points_free(s);
    if (rc) return rc;
    HIP_TRY(s.h_pts.ensure((size_t)n_points));
    HIP_TRY(s.d_pts.ensure((size_t)n_points));
    const size_t bytes = (size_t)n_points * sizeof(float4);
    tsdf_host::copy_to_pinned(s.h_pts.get(), points_host, bytes);
    HIP_TRY(hipMemcpyAsync(s.d_pts, s.h_pts, bytes, hipMemcpyHostToDevice, st));
    s.pts_in_use = true;            // (from here on, whatever fails: the copy is queued)
    return TSDF_OK;
}
tsdfk::ScanProjection scan_projection_of(const float velo2img[12], int H, int W)
{
    tsdfk::ScanProjection p;
    std::memcpy(p.m, velo2img, sizeof p.m);
    p.H = H; p.W = W;
    return p;
}

int scan_splat_points(ScanStage &s, const float velo2img[12], int H, int W, const float *points_host, int64_t n_points, hipStream_t st)
{
    int rc = scan_keys_ready(s, (size_t)H * W, st);
    if (rc || n_points == 0) return rc;
    rc = scan_upload_points(s, points_host, n_points, st);
    if (rc) return rc;
    s.keys_clean = false;
    hipLaunchKernelGGL(tsdfk::scan_splat, dim3(scan_blocks(n_points)), dim3(256), 0, st, scan_projection_of(velo2img, H, W), s.d_pts.get(),
                       n_points, s.d_keys.get());
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(s.pts_read, st));
    return TSDF_OK;
}

// The key image into a range and / or a depth image in HBM (either may be null), the keys back to zero.
int scan_resolve_keys(ScanStage &s, const tsdfk::ScanCamera k, int H, int W, float *range_dev, float *depth_dev, uint32_t *counts_dev,
                      hipStream_t st)
{
    hipLaunchKernelGGL(tsdfk::scan_resolve, dim3(scan_blocks((int64_t)H * W)), dim3(256), 0, st, k, H, W, s.d_keys.get(), range_dev,
                       depth_dev, counts_dev);
    HIP_TRY(hipGetLastError());
    s.keys_clean = true;
    return TSDF_OK;
}

int scanner_ensure(tsdf_scanner *s)
{
    if (s->d_images) return TSDF_OK;
    const size_t n_px = (size_t)s->H * s->W, nb = scan_blocks((int64_t)n_px);
    Stream st;
    DevPtr<float> d_images;
    DevPtr<uint32_t> d_counts;
    HostPtr<float> h_images;
    HIP_TRY(stream_create(st));
    HIP_TRY(dev_alloc(d_images, 2 * n_px * sizeof(float)));
    HIP_TRY(dev_alloc(d_counts, nb * sizeof(uint32_t)));
    HIP_TRY(host_alloc(h_images, 2 * n_px * sizeof(float) + nb * sizeof(uint32_t), hipHostMallocDefault));
    s->stream = std::move(st); s->d_images = std::move(d_images); s->d_counts = std::move(d_counts); s->h_images = std::move(h_images);
    return TSDF_OK;
}

// The handle's camera for the lidar entry points: tsdf_create does not look at cam_K, the conversion divides by fx and fy.
int scan_volume_ok(const char *who, const tsdf_volume *v)
{
    int rc = scan_camera_ok(who, v->cfg.cam_K);
    if (rc) return rc;
    return image_ok(who, v->cfg.im_height, v->cfg.im_width);
}

}  // namespace

extern "C" {

int tsdf_scan_projection(const float P_rect[12], const float R_rect[9], const float R_velo[9], const float t_velo[3],
                         float velo2img_out[12])
{
    if (!P_rect || !R_rect || !R_velo || !t_velo || !velo2img_out) return fail(TSDF_ERR_INVALID, "tsdf_scan_projection: NULL argument");
    // ref: src/Utility.cpp:42-49 -- P_rect * [R_rect 0; 0 1] * [R_velo t_velo; 0 1], each entry a left-to-right sum
    float a[16] = {0}, b[16] = {0}, p[16] = {0}, ab[16], out[16];
    for (int r = 0; r < 3; ++r) {
        for (int c = 0; c < 3; ++c) { a[4 * r + c] = R_rect[3 * r + c]; b[4 * r + c] = R_velo[3 * r + c]; }
        b[4 * r + 3] = t_velo[r];
        for (int c = 0; c < 4; ++c) p[4 * r + c] = P_rect[4 * r + c];
    }
    a[15] = b[15] = 1.0f;      // (p's fourth row stays zero and is dropped)
    tsdf_host::multiply_matrix(p, a, ab);
    tsdf_host::multiply_matrix(ab, b, out);
    std::memcpy(velo2img_out, out, 12 * sizeof(float));
    return TSDF_OK;
}

int tsdf_scanner_destroy(tsdf_scanner *s)
{
    if (!s) return TSDF_OK;
    (void)hipSetDevice(s->device);
    if (s->stream) (void)hipStreamSynchronize(s->stream);
    delete s;            // the owners release the memory and the stream (the device is current)
    return TSDF_OK;
}

int tsdf_scanner_create(int32_t device, int32_t im_height, int32_t im_width, tsdf_scanner **out)
{
    const char *who = "tsdf_scanner_create";
    if (!out) return fail(TSDF_ERR_INVALID, "%s: NULL argument", who);
    *out = nullptr;
    int rc = image_ok(who, im_height, im_width);
    if (rc) return rc;
    int n_dev = 0;
    if (hipGetDeviceCount(&n_dev) != hipSuccess || n_dev <= 0)
        return fail(TSDF_ERR_NO_DEVICE, "%s: no HIP device visible (this library has no CPU path)", who);
    if (device < 0 || device >= n_dev) return fail(TSDF_ERR_INVALID, "%s: device %d not in [0,%d)", who, device, n_dev);
    tsdf_scanner *s = new (std::nothrow) tsdf_scanner();
    if (!s) return fail(TSDF_ERR_INVALID, "%s: out of host memory", who);
    s->device = device; s->H = im_height; s->W = im_width;
    *out = s;
    return TSDF_OK;
}

int tsdf_scan_project(tsdf_scanner *s, const float velo2img[12], const float cam_K[9], const float *points_host, int64_t n_points,
                      float *range_host, float *depth_host, int64_t *n_pixels)
{
    const char *who = "tsdf_scan_project";
    if (!s || !velo2img || (depth_host && !cam_K)) return fail(TSDF_ERR_INVALID, "%s: NULL argument", who);
    if (!range_host && !depth_host && !n_pixels) return fail(TSDF_ERR_INVALID, "%s: NULL argument (all three outputs)", who);
    int rc = scan_points_ok(who, points_host, n_points);
    if (rc == TSDF_OK) rc = scan_matrix_ok(who, "velo2img", velo2img, 12);
    if (rc == TSDF_OK && depth_host) rc = scan_camera_ok(who, cam_K);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(s->device));
    rc = scanner_ensure(s);
    if (rc) return rc;
    const size_t n_px = (size_t)s->H * s->W, nb = scan_blocks((int64_t)n_px);
    rc = scan_splat_points(s->stage, velo2img, s->H, s->W, points_host, n_points, s->stream);
    if (rc) return rc;
    float *d_range = s->d_images.get(), *d_depth = d_range + n_px, *h_range = s->h_images.get(), *h_depth = h_range + n_px;
    uint32_t *h_counts = reinterpret_cast<uint32_t *>(h_depth + n_px);
    const tsdfk::ScanCamera k = depth_host ? scan_camera(cam_K) : tsdfk::ScanCamera{1.0f, 1.0f, 0.0f, 0.0f};
    rc = scan_resolve_keys(s->stage, k, s->H, s->W, range_host ? d_range : nullptr, depth_host ? d_depth : nullptr,
                           n_pixels ? s->d_counts.get() : nullptr, s->stream);
    if (rc) return rc;
    if (range_host) HIP_TRY(hipMemcpyAsync(h_range, d_range, n_px * sizeof(float), hipMemcpyDeviceToHost, s->stream));
    if (depth_host) HIP_TRY(hipMemcpyAsync(h_depth, d_depth, n_px * sizeof(float), hipMemcpyDeviceToHost, s->stream));
    if (n_pixels) HIP_TRY(hipMemcpyAsync(h_counts, s->d_counts, nb * sizeof(uint32_t), hipMemcpyDeviceToHost, s->stream));
    HIP_TRY(hipStreamSynchronize(s->stream));
    if (range_host) std::memcpy(range_host, h_range, n_px * sizeof(float));
    if (depth_host) std::memcpy(depth_host, h_depth, n_px * sizeof(float));
    if (n_pixels) {
        int64_t total = 0;
        for (size_t b = 0; b < nb; ++b) total += h_counts[b];
        *n_pixels = total;
    }
    return TSDF_OK;
}

int tsdf_scan_range_to_depth(tsdf_scanner *s, const float cam_K[9], const float *range_host, float *depth_host)
{
    const char *who = "tsdf_scan_range_to_depth";
    if (!s || !cam_K || !range_host || !depth_host) return fail(TSDF_ERR_INVALID, "%s: NULL argument", who);
    int rc = scan_camera_ok(who, cam_K);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(s->device));
    rc = scanner_ensure(s);
    if (rc) return rc;
    const size_t n_px = (size_t)s->H * s->W, img = n_px * sizeof(float);
    float *d_range = s->d_images.get(), *d_depth = d_range + n_px, *h_range = s->h_images.get(), *h_depth = h_range + n_px;
    tsdf_host::copy_to_pinned(h_range, range_host, img);
    HIP_TRY(hipMemcpyAsync(d_range, h_range, img, hipMemcpyHostToDevice, s->stream));
    hipLaunchKernelGGL(tsdfk::scan_range_to_depth, dim3(scan_blocks((int64_t)n_px)), dim3(256), 0, s->stream, scan_camera(cam_K), s->H,
                       s->W, d_range, d_depth);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(h_depth, d_depth, img, hipMemcpyDeviceToHost, s->stream));
    HIP_TRY(hipStreamSynchronize(s->stream));
    std::memcpy(depth_host, h_depth, img);
    return TSDF_OK;
}

int tsdf_integrate_range(tsdf_volume *v, const float *range_host, const float cam2world[16])
{
    const char *who = "tsdf_integrate_range";
    if (!v || !range_host || !cam2world) return fail(TSDF_ERR_INVALID, "%s: NULL argument", who);
    int rc = scan_volume_ok(who, v);
    if (rc) return rc;
    const bool defer = v->defer_n > 1;
    rc = bind_device(v, !defer);
    if (rc) return rc;
    // as stage_frame_u16: the ranges are staged into a slot of their own and converted on the copy stream into the frame's
    const int H = v->cfg.im_height, W = v->cfg.im_width;
    const size_t img = (size_t)H * W * sizeof(float);
    StoreSlot raw, frame;
    rc = stage_frame(v, img, [&](float *pinned) { tsdf_host::copy_to_pinned(pinned, range_host, img); }, raw);
    if (rc == TSDF_OK) rc = frame.take(v, &v->store->frames, v->copy_stream);
    if (rc) return rc;
    hipLaunchKernelGGL(tsdfk::scan_range_to_depth, dim3(scan_blocks((int64_t)H * W)), dim3(256), 0, v->copy_stream,
                       scan_camera(v->cfg.cam_K), H, W, raw.as<float>(), frame.as<float>());
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(v->pend_copied, v->copy_stream));
    raw.release_after(&v->pend_copied);
    return apply_host_frame(v, frame, cam2world, defer, true);
}

int tsdf_integrate_scan(tsdf_volume *v, const float velo2img[12], const float *points_host, int64_t n_points, const float cam2world[16])
{
    const char *who = "tsdf_integrate_scan";
    if (!v || !velo2img || !cam2world) return fail(TSDF_ERR_INVALID, "%s: NULL argument", who);
    int rc = scan_points_ok(who, points_host, n_points);
    if (rc == TSDF_OK) rc = scan_matrix_ok(who, "velo2img", velo2img, 12);
    if (rc == TSDF_OK) rc = scan_volume_ok(who, v);
    if (rc) return rc;
    const bool defer = v->defer_n > 1;
    rc = bind_device(v, !defer);
    if (rc) return rc;
    // points -> keys -> the frame's slot of the store, all on the copy stream: the image never leaves the device
    const int H = v->cfg.im_height, W = v->cfg.im_width;
    rc = scan_splat_points(v->scan, velo2img, H, W, points_host, n_points, v->copy_stream);
    if (rc) return rc;
    StoreSlot frame;
    rc = frame.take(v, &v->store->frames, v->copy_stream);
    if (rc) return rc;
    rc = scan_resolve_keys(v->scan, scan_camera(v->cfg.cam_K), H, W, nullptr, frame.as<float>(), nullptr, v->copy_stream);
    if (rc) return rc;
    HIP_TRY(hipEventRecord(v->pend_copied, v->copy_stream));
    return apply_host_frame(v, frame, cam2world, defer, true);
}

}  // extern "C"
