// tsdf_scan_ground_host.hip.h -- host side of marking a scan's ground (tsdf_scan_ground_params_default, tsdf_scan_mark_ground,
// tsdf_scan_project_ground, tsdf_integrate_scan_ground; tsdf_scan_ground.hip.h states the rule, scan_ground_tables.h builds its
// tables), included at the end of tsdf_capi.hip after the gap fill's host header, whose scanner, checks and staging it shares.
#pragma once

namespace {

int scan_ground_params_ok(const char *who, const tsdf_scan_ground_params *p)
{
    const tsdf_host::GroundLimit l = tsdf_host::scan_ground_limits_ok(*p);
    if (l != tsdf_host::GroundLimit::Ok) return fail(TSDF_ERR_INVALID, "%s: ground_params: %s", who, tsdf_host::ground_limit_text(l));
    return TSDF_OK;
}

int scan_select_ok(const char *who, int32_t select)
{
    if (select != TSDF_SCAN_DROP_GROUND && select != TSDF_SCAN_ONLY_GROUND)
        return fail(TSDF_ERR_INVALID, "%s: select = %d is neither TSDF_SCAN_DROP_GROUND nor TSDF_SCAN_ONLY_GROUND", who, select);
    return TSDF_OK;
}

// The counting kernels' words in d_counts: one per workgroup of ground_splat | two per workgroup of ground_mark | one per
// workgroup of ground_flags or scan_splat_select.
struct GroundCounts {
    size_t nb_pts, nb_cells;
    size_t words() const { return 2 * nb_pts + 2 * nb_cells; }
    size_t mark() const { return nb_pts; }
    size_t tail() const { return nb_pts + 2 * nb_cells; }
};
GroundCounts ground_counts(const tsdf_scan_ground_params &p, int64_t n_points)
{
    GroundCounts c;
    c.nb_pts = scan_blocks(n_points);
    c.nb_cells = (size_t)scan_blocks(p.n_columns) * (size_t)p.n_rings;
    return c;
}

// The stage made ready for a scan of n_points under p: the tables of p in HBM (rebuilt and queued on `st` when p is not the
// last call's), every buffer large enough.  The caller has waited for the last scan's kernels (scan_points_free).
int ground_prepare(const char *who, ScanGroundStage &g, const tsdf_scan_ground_params &p, int64_t n_points, bool want_winner,
                   bool want_flags, hipStream_t st)
{
    const size_t n_cells = (size_t)p.n_rings * p.n_columns, n_tab = (size_t)p.n_rings + 1 + 2 * (size_t)p.n_columns;
    if (!g.have_tables || std::memcmp(&g.params, &p, sizeof p) != 0) {
        g.have_tables = false;
        const tsdf_host::GroundLimit l = tsdf_host::build_scan_ground_tables(p, g.tables);
        if (l != tsdf_host::GroundLimit::Ok) return fail(TSDF_ERR_INVALID, "%s: ground_params: %s", who, tsdf_host::ground_limit_text(l));
        HIP_TRY(g.h_tables.ensure(n_tab));
        HIP_TRY(g.d_tables.ensure(n_tab));
        float *h = g.h_tables.get();
        std::memcpy(h, g.tables.T.data(), ((size_t)p.n_rings + 1) * sizeof(float));
        std::memcpy(h + p.n_rings + 1, g.tables.C.data(), (size_t)p.n_columns * sizeof(float));
        std::memcpy(h + p.n_rings + 1 + p.n_columns, g.tables.S.data(), (size_t)p.n_columns * sizeof(float));
        HIP_TRY(hipMemcpyAsync(g.d_tables, g.h_tables, n_tab * sizeof(float), hipMemcpyHostToDevice, st));
        g.params = p;
        g.have_tables = true;
    }
    if (!g.d_keys.fits(n_cells)) { HIP_TRY(g.d_keys.ensure(n_cells)); g.keys_clean = false; }
    HIP_TRY(g.d_state.ensure(n_cells));
    if (want_winner) HIP_TRY(g.d_winner.ensure(n_cells));
    HIP_TRY(g.d_cells.ensure((size_t)std::max<int64_t>(n_points, 1)));
    if (want_flags) HIP_TRY(g.d_flags.ensure((size_t)std::max<int64_t>(n_points, 1)));
    HIP_TRY(g.d_counts.ensure(ground_counts(p, n_points).words()));
    return TSDF_OK;
}

tsdfk::ScanGround ground_args(const ScanGroundStage &g)
{
    const tsdf_scan_ground_params &p = g.params;
    tsdfk::ScanGround a;
    a.n_rings = p.n_rings; a.n_columns = p.n_columns; a.ground_rings = p.ground_rings; a.mark_upper = p.mark_upper;
    a.min_range = p.min_range; a.tlo = g.tables.tlo; a.thi = g.tables.thi;
    for (int q = 0; q < 4; ++q) { a.first[q] = g.tables.first[q]; a.len[q] = g.tables.len[q]; }
    a.T = g.d_tables.get(); a.C = a.T + p.n_rings + 1; a.S = a.C + p.n_columns;
    return a;
}

// The points in s.d_pts -> their cells and the cells' keys -> the cells' states, queued on `st`; the spherical key image is
// cleared again behind ground_mark by a memset (ground_mark reads the rows above and below a workgroup's own, so it cannot
// clear what it reads as scan_resolve does; 8 bytes x n_rings x n_columns, 2.3 MB at 64 x 4500).  counted: the workgroups'
// counts into d_counts.
int ground_mark_launch(ScanStage &s, ScanGroundStage &g, int64_t n_points, bool want_winner, bool counted, hipStream_t st)
{
    const tsdf_scan_ground_params &p = g.params;
    const size_t key_bytes = (size_t)p.n_rings * p.n_columns * sizeof(unsigned long long);
    const GroundCounts gc = ground_counts(p, n_points);
    const tsdfk::ScanGround a = ground_args(g);
    uint32_t *counts = counted ? g.d_counts.get() : nullptr;
    // not clean: a call failed between the splat and the clear below, under whatever grid it had -- the whole buffer is cleared
    if (!g.keys_clean) HIP_TRY(hipMemsetAsync(g.d_keys, 0, g.d_keys.capacity() * sizeof(unsigned long long), st));
    g.keys_clean = true;
    if (n_points > 0) {
        g.keys_clean = false;
        hipLaunchKernelGGL(tsdfk::ground_splat, dim3((unsigned)gc.nb_pts), dim3(256), 0, st, a, s.d_pts.get(), n_points, g.d_keys.get(),
                           g.d_cells.get(), counts);
        HIP_TRY(hipGetLastError());
    }
    hipLaunchKernelGGL(tsdfk::ground_mark, dim3(scan_blocks(p.n_columns), (unsigned)p.n_rings), dim3(256), 0, st, a, g.d_keys.get(),
                       s.d_pts.get(), n_points, g.d_state.get(), want_winner ? g.d_winner.get() : nullptr,
                       counts ? counts + gc.mark() : nullptr);
    HIP_TRY(hipGetLastError());
    if (n_points > 0) {
        HIP_TRY(hipMemsetAsync(g.d_keys, 0, key_bytes, st));
        g.keys_clean = true;
    }
    return TSDF_OK;
}

// scan_splat_points for the points `select` keeps: the camera's key image ready, the points in HBM, marked, and the kept ones
// splatted, all queued on `st`.  count_kept: the workgroups' numbers of kept points into the tail of g.d_counts.
int scan_splat_selected(const char *who, ScanStage &s, ScanGroundStage &g, const float velo2img[12], int H, int W,
                        const tsdf_scan_ground_params &gp, int32_t select, const float *points_host, int64_t n_points, bool count_kept,
                        hipStream_t st)
{
    int rc = scan_keys_ready(s, (size_t)H * W, st);
    if (rc || n_points == 0) return rc;
    rc = scan_points_free(s);            // in front of anything of the ground stage that is regrown or refilled
    if (rc == TSDF_OK) rc = ground_prepare(who, g, gp, n_points, false, false, st);
    if (rc == TSDF_OK) rc = scan_upload_points(s, points_host, n_points, st);
    if (rc == TSDF_OK) rc = ground_mark_launch(s, g, n_points, false, false, st);
    if (rc) return rc;
    s.keys_clean = false;
    hipLaunchKernelGGL(tsdfk::scan_splat_select, dim3(scan_blocks(n_points)), dim3(256), 0, st, scan_projection_of(velo2img, H, W),
                       s.d_pts.get(), n_points, s.d_keys.get(), g.d_cells.get(), g.d_state.get(), select == TSDF_SCAN_ONLY_GROUND ? 1 : 0,
                       count_kept ? g.d_counts.get() + ground_counts(gp, n_points).tail() : nullptr);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(s.pts_read, st));
    return TSDF_OK;
}

int64_t sum_words(const uint32_t *w, size_t n, size_t stride = 1)
{
    int64_t total = 0;
    for (size_t i = 0; i < n; ++i) total += w[i * stride];
    return total;
}

}  // namespace

extern "C" {

int tsdf_scan_ground_params_default(tsdf_scan_ground_params *out)
{
    if (!out) return fail(TSDF_ERR_INVALID, "tsdf_scan_ground_params_default: NULL argument");
    out->n_rings = 64;                   // ref: include/Utility.hpp:52-58 (N_SCAN, Horizon_SCAN, ang_res_y, ang_bottom,
    out->n_columns = 4500;               // sensorMountAngle), src/Utility.cpp:484 (range < 0.1), :529 (<= 2.5)
    out->ang_res_y = 26.9f / 63.0f;
    out->ang_bottom = 15.1f;
    out->mount_deg = 0.0f;
    out->tol_deg = 2.5f;
    out->min_range = 0.1f;
    out->ground_rings = 63;              // the reference's loop without its last row, which reads past the image
    out->mark_upper = 0;                 // ref: :531 is commented out
    return TSDF_OK;
}

int tsdf_scan_mark_ground(tsdf_scanner *s, const tsdf_scan_ground_params *params, const float *points_host, int64_t n_points,
                          uint8_t *flags_host, int8_t *state_host, int32_t *winner_host, int64_t counts[4])
{
    const char *who = "tsdf_scan_mark_ground";
    if (!s || !params) return fail(TSDF_ERR_INVALID, "%s: NULL argument", who);
    if (!flags_host && !state_host && !winner_host && !counts) return fail(TSDF_ERR_INVALID, "%s: NULL argument (all four outputs)", who);
    int rc = scan_points_ok(who, points_host, n_points);
    if (rc == TSDF_OK) rc = scan_ground_params_ok(who, params);
    if (rc) return rc;
    if (winner_host && n_points > INT32_MAX)
        return fail(TSDF_ERR_INVALID, "%s: n_points = %lld does not fit winner_host's 32-bit indices", who, (long long)n_points);
    HIP_TRY(hipSetDevice(s->device));
    rc = scanner_ensure(s);
    if (rc) return rc;
    ScanGroundStage &g = s->ground;
    const bool pointwise = flags_host || counts;
    rc = scan_points_free(s->stage);
    if (rc == TSDF_OK) rc = ground_prepare(who, g, *params, n_points, winner_host != nullptr, flags_host != nullptr, s->stream);
    if (rc == TSDF_OK && n_points > 0) rc = scan_upload_points(s->stage, points_host, n_points, s->stream);
    if (rc == TSDF_OK) rc = ground_mark_launch(s->stage, g, n_points, winner_host != nullptr, counts != nullptr, s->stream);
    if (rc) return rc;
    const GroundCounts gc = ground_counts(*params, n_points);
    if (pointwise && n_points > 0) {
        hipLaunchKernelGGL(tsdfk::ground_flags, dim3((unsigned)gc.nb_pts), dim3(256), 0, s->stream, g.d_cells.get(), g.d_state.get(), n_points,
                           flags_host ? g.d_flags.get() : nullptr, counts ? g.d_counts.get() + gc.tail() : nullptr);
        HIP_TRY(hipGetLastError());
    }
    if (n_points > 0) HIP_TRY(hipEventRecord(s->stage.pts_read, s->stream));
    // back through the pinned block: states | winners | counts | flags (each part 4-byte aligned but the last)
    const size_t n_cells = (size_t)params->n_rings * params->n_columns, state_bytes = (n_cells + 3) / 4 * 4;
    HIP_TRY(g.h_out.ensure(state_bytes + n_cells * sizeof(int32_t) + gc.words() * sizeof(uint32_t) + (size_t)n_points));
    char *h_state = g.h_out.get(), *h_winner = h_state + state_bytes, *h_counts = h_winner + n_cells * sizeof(int32_t);
    char *h_flags = h_counts + gc.words() * sizeof(uint32_t);
    if (state_host) HIP_TRY(hipMemcpyAsync(h_state, g.d_state, n_cells, hipMemcpyDeviceToHost, s->stream));
    if (winner_host) HIP_TRY(hipMemcpyAsync(h_winner, g.d_winner, n_cells * sizeof(int32_t), hipMemcpyDeviceToHost, s->stream));
    if (counts) HIP_TRY(hipMemcpyAsync(h_counts, g.d_counts, gc.words() * sizeof(uint32_t), hipMemcpyDeviceToHost, s->stream));
    if (flags_host && n_points > 0) HIP_TRY(hipMemcpyAsync(h_flags, g.d_flags, (size_t)n_points, hipMemcpyDeviceToHost, s->stream));
    HIP_TRY(hipStreamSynchronize(s->stream));
    if (state_host) std::memcpy(state_host, h_state, n_cells);
    if (winner_host) std::memcpy(winner_host, h_winner, n_cells * sizeof(int32_t));
    if (flags_host && n_points > 0) std::memcpy(flags_host, h_flags, (size_t)n_points);
    if (counts) {
        const uint32_t *w = reinterpret_cast<const uint32_t *>(h_counts);
        counts[0] = sum_words(w, gc.nb_pts);
        counts[1] = sum_words(w + gc.mark(), gc.nb_cells, 2);
        counts[2] = sum_words(w + gc.mark() + 1, gc.nb_cells, 2);
        counts[3] = sum_words(w + gc.tail(), gc.nb_pts);
    }
    return TSDF_OK;
}

int tsdf_scan_project_ground(tsdf_scanner *s, const float velo2img[12], const float cam_K[9], const tsdf_scan_ground_params *ground_params,
                             int32_t select, const tsdf_scan_fill_params *fill_params, const float *points_host, int64_t n_points,
                             float *range_host, float *depth_host, uint8_t *kind_host, int64_t *n_pixels, int64_t *n_filled,
                             int64_t *n_selected)
{
    const char *who = "tsdf_scan_project_ground";
    const bool wants_depth = depth_host || kind_host || n_filled;          // what needs the z-depth image on the device
    if (!s || !velo2img || !ground_params || (wants_depth && !cam_K)) return fail(TSDF_ERR_INVALID, "%s: NULL argument", who);
    if (!range_host && !depth_host && !kind_host && !n_pixels && !n_filled && !n_selected)
        return fail(TSDF_ERR_INVALID, "%s: NULL argument (all six outputs)", who);
    if (!fill_params && (kind_host || n_filled)) return fail(TSDF_ERR_INVALID, "%s: kind_host and n_filled need fill_params", who);
    int rc = scan_points_ok(who, points_host, n_points);
    if (rc == TSDF_OK) rc = scan_matrix_ok(who, "velo2img", velo2img, 12);
    if (rc == TSDF_OK && wants_depth) rc = scan_camera_ok(who, cam_K);
    if (rc == TSDF_OK) rc = scan_ground_params_ok(who, ground_params);
    if (rc == TSDF_OK) rc = scan_select_ok(who, select);
    if (rc == TSDF_OK && fill_params) rc = scan_fill_params_ok(who, fill_params);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(s->device));
    const bool fills = fill_params && wants_depth;
    rc = fills ? scanner_fill_ensure(s) : scanner_ensure(s);
    if (rc) return rc;
    ScanGroundStage &g = s->ground;
    // points -> ground states -> the kept points' keys -> range and sparse depth (-> the filled depth), all in HBM
    rc = scan_splat_selected(who, s->stage, g, velo2img, s->H, s->W, *ground_params, select, points_host, n_points, n_selected != nullptr,
                             s->stream);
    if (rc) return rc;
    const size_t n_px = (size_t)s->H * s->W, nb = scan_blocks((int64_t)n_px), nb_pts = scan_blocks(n_points);
    float *d_range = s->d_images.get(), *d_depth = d_range + n_px, *h_range = s->h_images.get(), *h_depth = h_range + n_px;
    uint32_t *h_counts = reinterpret_cast<uint32_t *>(h_depth + n_px);
    const tsdfk::ScanCamera k = wants_depth ? scan_camera(cam_K) : tsdfk::ScanCamera{1.0f, 1.0f, 0.0f, 0.0f};
    rc = scan_resolve_keys(s->stage, k, s->H, s->W, range_host ? d_range : nullptr, wants_depth ? d_depth : nullptr,
                           n_pixels ? s->d_counts.get() : nullptr, s->stream);
    if (rc) return rc;
    if (range_host) HIP_TRY(hipMemcpyAsync(h_range, d_range, n_px * sizeof(float), hipMemcpyDeviceToHost, s->stream));
    if (depth_host && !fills) HIP_TRY(hipMemcpyAsync(h_depth, d_depth, n_px * sizeof(float), hipMemcpyDeviceToHost, s->stream));
    if (n_pixels) HIP_TRY(hipMemcpyAsync(h_counts, s->d_counts, nb * sizeof(uint32_t), hipMemcpyDeviceToHost, s->stream));
    if (n_selected && n_points > 0) {
        HIP_TRY(g.h_out.ensure(nb_pts * sizeof(uint32_t)));
        HIP_TRY(hipMemcpyAsync(g.h_out, g.d_counts.get() + ground_counts(*ground_params, n_points).tail(), nb_pts * sizeof(uint32_t),
                               hipMemcpyDeviceToHost, s->stream));
    }
    if (fills) {
        rc = scanner_fill_and_fetch(s, *fill_params, depth_host, kind_host, n_filled);      // (synchronises the stream)
        if (rc) return rc;
    } else {
        HIP_TRY(hipStreamSynchronize(s->stream));
        if (depth_host) std::memcpy(depth_host, h_depth, n_px * sizeof(float));
    }
    if (range_host) std::memcpy(range_host, h_range, n_px * sizeof(float));
    if (n_pixels) *n_pixels = sum_words(h_counts, nb);
    if (n_selected) *n_selected = n_points > 0 ? sum_words(reinterpret_cast<const uint32_t *>(g.h_out.get()), nb_pts) : 0;
    return TSDF_OK;
}

int tsdf_integrate_scan_ground(tsdf_volume *v, const float velo2img[12], const tsdf_scan_ground_params *ground_params, int32_t select,
                               const tsdf_scan_fill_params *fill_params, const float *points_host, int64_t n_points,
                               const float cam2world[16])
{
    const char *who = "tsdf_integrate_scan_ground";
    if (!v || !velo2img || !ground_params || !cam2world) return fail(TSDF_ERR_INVALID, "%s: NULL argument", who);
    int rc = scan_points_ok(who, points_host, n_points);
    if (rc == TSDF_OK) rc = scan_matrix_ok(who, "velo2img", velo2img, 12);
    if (rc == TSDF_OK) rc = scan_volume_ok(who, v);
    if (rc == TSDF_OK) rc = scan_ground_params_ok(who, ground_params);
    if (rc == TSDF_OK) rc = scan_select_ok(who, select);
    if (rc == TSDF_OK && fill_params) rc = scan_fill_params_ok(who, fill_params);
    if (rc) return rc;
    const bool defer = v->defer_n > 1;
    rc = bind_device(v, !defer);
    if (rc) return rc;
    // as tsdf_integrate_scan / _filled with the marking and the selecting splat in place of scan_splat, all on the copy stream
    const int H = v->cfg.im_height, W = v->cfg.im_width;
    rc = scan_splat_selected(who, v->scan, v->ground, velo2img, H, W, *ground_params, select, points_host, n_points, false, v->copy_stream);
    if (rc) return rc;
    StoreSlot sparse, frame;
    if (fill_params) rc = sparse.take(v, &v->store->frames, v->copy_stream);
    if (rc == TSDF_OK) rc = frame.take(v, &v->store->frames, v->copy_stream);
    if (rc) return rc;
    rc = scan_resolve_keys(v->scan, scan_camera(v->cfg.cam_K), H, W, nullptr, (fill_params ? sparse : frame).as<float>(), nullptr,
                           v->copy_stream);
    if (rc == TSDF_OK && fill_params)
        rc = scan_fill_launch(*fill_params, H, W, sparse.as<float>(), frame.as<float>(), nullptr, nullptr, v->copy_stream);
    if (rc) return rc;
    HIP_TRY(hipEventRecord(v->pend_copied, v->copy_stream));
    if (fill_params) sparse.release_after(&v->pend_copied);
    return apply_host_frame(v, frame, cam2world, defer, true);
}

}  // extern "C"
