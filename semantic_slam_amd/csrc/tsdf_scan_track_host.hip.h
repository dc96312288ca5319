// tsdf_scan_track_host.hip.h -- host side of tracking a scan against the volume (include/tsdf_hip.h: tsdf_scan_track*,
// tsdf_scan_pose), included at the end of tsdf_capi.hip after tsdf_track_host.hip.h, whose state and handle checks it uses, and
// after the lidar host headers, whose points' staging it shares; tsdf_scan_track.hip.h states the rule.
#pragma once

namespace {

int scan_track_params_ok(const char *who, const tsdf_scan_track_params *p)
{
    if (!std::isfinite(p->weight_thresh)) return fail(TSDF_ERR_INVALID, "%s: weight_thresh is not finite", who);
    if (!(std::isfinite(p->resid_thresh) && p->resid_thresh > 0.0f))
        return fail(TSDF_ERR_INVALID, "%s: resid_thresh must be finite and > 0 (%g)", who, (double)p->resid_thresh);
    if (!(std::isfinite(p->min_range_m) && std::isfinite(p->max_range_m) && p->min_range_m >= 0.0f && p->min_range_m <= p->max_range_m))
        return fail(TSDF_ERR_INVALID, "%s: min_range_m and max_range_m must be finite with 0 <= min <= max (%g, %g)", who,
                    (double)p->min_range_m, (double)p->max_range_m);
    if (p->n_levels < 1 || p->n_levels > 3) return fail(TSDF_ERR_INVALID, "%s: n_levels %d is outside 1..3", who, p->n_levels);
    for (int l = 0; l < p->n_levels; ++l)
        if (p->iters[l] < 0) return fail(TSDF_ERR_INVALID, "%s: iters[%d] = %d is negative", who, l, p->iters[l]);
    if (p->min_pairs < 0) return fail(TSDF_ERR_INVALID, "%s: min_pairs %d is negative", who, p->min_pairs);
    if (p->drop_flag < -1 || p->drop_flag > 255) return fail(TSDF_ERR_INVALID, "%s: drop_flag %d is outside -1..255", who, p->drop_flag);
    if (!(std::isfinite(p->eps_rot) && p->eps_rot > 0.0f && std::isfinite(p->eps_trans) && p->eps_trans > 0.0f))
        return fail(TSDF_ERR_INVALID, "%s: eps_rot and eps_trans must be finite and > 0 (%g, %g)", who, (double)p->eps_rot,
                    (double)p->eps_trans);
    return TSDF_OK;
}

// Everything refused before anything is queued; then the collected frames.
int scan_track_checks(const char *who, tsdf_volume *v, const tsdf_scan_track_params *p, const float *points_host, int64_t n_points,
                      const char *pose_name, const float *pose, const void *out)
{
    if (!v || !p || !pose) return fail(TSDF_ERR_INVALID, "%s: NULL argument", who);
    if (!out) return fail(TSDF_ERR_INVALID, "%s: NULL result", who);
    // one lane per point at level 0, in whole wavefronts
    if (n_points < 0 || n_points > ((int64_t)1 << 31) - 64)
        return fail(TSDF_ERR_INVALID, "%s: n_points = %lld is outside [0, 2^31 - 64] (one lane per point in one pass)", who,
                    (long long)n_points);
    if (n_points > 0 && !points_host) return fail(TSDF_ERR_INVALID, "%s: NULL points_host with n_points = %lld", who, (long long)n_points);
    if (v->group_owner) return fail(TSDF_ERR_INVALID, "%s: the handle is a slab of a tsdf_group; tracking needs a whole-grid handle", who);
    int rc = ray_volume_ok(who, v);                       // a whole-grid handle, every dim >= 2
    if (rc == TSDF_OK) rc = scan_track_params_ok(who, p);
    if (rc == TSDF_OK) rc = scan_matrix_ok(who, pose_name, pose, 12);
    if (rc) return rc;
    return bind_device(v);   // the collected frames first
}

// The scratch block: partial rows | state, and the state's pinned copy; no size of the scan enters it.
struct ScanTrackScratch {
    double *partials;
    tsdfk::TrackState *state;
};

int scan_track_scratch(tsdf_volume *v, ScanTrackScratch *sc)
{
    tsdf_host::Regions r;
    const size_t o_p = r.add(sizeof(double) * tsdfk::kTrackMaxBlocks * tsdfk::kTrackTerms);
    const size_t o_s = r.add(sizeof(tsdfk::TrackState));
    if (!v->h_scan_track) HIP_TRY(host_alloc(v->h_scan_track, sizeof(tsdfk::TrackState), hipHostMallocDefault));
    HIP_TRY(v->d_scan_track.ensure(r.total()));
    char *base = v->d_scan_track;
    sc->partials = reinterpret_cast<double *>(base + o_p);
    sc->state = reinterpret_cast<tsdfk::TrackState *>(base + o_s);
    return TSDF_OK;
}

// The scan into the handle's scan memory and the flags beside it, queued on the handle's stream.  The flags' two blocks are
// free whenever a call begins: every call that fills them returns behind the stream.
int scan_track_upload(tsdf_volume *v, const float *points_host, const uint8_t *flags_host, int64_t n_points)
{
    if (n_points == 0) return TSDF_OK;
    int rc = scan_upload_points(v->scan, points_host, n_points, v->stream);
    if (rc || !flags_host) return rc;
    HIP_TRY(v->h_scan_flags.ensure((size_t)n_points));
    HIP_TRY(v->d_scan_flags.ensure((size_t)n_points));
    std::memcpy(v->h_scan_flags.get(), flags_host, (size_t)n_points);
    HIP_TRY(hipMemcpyAsync(v->d_scan_flags, v->h_scan_flags, (size_t)n_points, hipMemcpyHostToDevice, v->stream));
    return TSDF_OK;
}

// One pass of level `level` as scan_track_pairs reads it, and its grid.
tsdfk::ScanTrackPairsParams scan_track_pairs_params(const tsdf_volume *v, const tsdf_scan_track_params *p, const ScanTrackScratch &sc,
                                                    int64_t n_points, bool flags, int level, int *n_blocks)
{
    const tsdf_config &c = v->cfg;
    const int s = 1 << level;
    tsdfk::ScanTrackPairsParams k;
    k.pts = v->scan.d_pts.get();
    k.flags = flags && n_points > 0 ? v->d_scan_flags.get() : nullptr;
    k.t = v->d_tsdf; k.w = v->d_weight;
    k.state = sc.state; k.partials = sc.partials;
    const int dims[3] = {c.dim_x, c.dim_y, c.dim_z};
    for (int i = 0; i < 3; ++i) {
        k.org[i] = c.origin[i];
        k.hi[i] = (float)(dims[i] - 1);
        k.dim[i] = dims[i];
    }
    k.vs = c.voxel_size;
    const int64_t n_sel = (n_points + s - 1) / s, lanes = (n_sel + 63) / 64 * 64;
    k.n_sel = (unsigned)n_sel;
    k.n_lanes = (unsigned)lanes;
    k.s = s; k.level = level;
    k.drop = p->drop_flag;
    k.rmin2 = p->min_range_m * p->min_range_m;
    k.rmax2 = p->max_range_m * p->max_range_m;
    k.tr = c.trunc_margin;
    k.gscale = c.trunc_margin / c.voxel_size;
    k.wthr = p->weight_thresh; k.rthr = p->resid_thresh;
    *n_blocks = (int)std::max<int64_t>(1, std::min<int64_t>((lanes + 255) / 256, tsdfk::kTrackMaxBlocks));
    return k;
}

// One iteration of level `level` on the handle's stream: the pair pass and the solve (system_only: the summed system, no step).
int scan_track_iteration(tsdf_volume *v, const tsdf_scan_track_params *p, const ScanTrackScratch &sc, int64_t n_points, bool flags,
                         int level, bool system_only)
{
    int nb = 0;
    const tsdfk::ScanTrackPairsParams k = scan_track_pairs_params(v, p, sc, n_points, flags, level, &nb);
    hipLaunchKernelGGL(tsdfk::scan_track_pairs, dim3(nb), dim3(256), 0, v->stream, k);
    HIP_TRY(hipGetLastError());
    tsdfk::TrackSolveParams q;
    q.state = sc.state; q.partials = sc.partials; q.n_rows = nb; q.level = level; q.min_inliers = p->min_pairs;
    q.system_only = system_only ? 1 : 0;
    q.eps_rot = p->eps_rot; q.eps_trans = p->eps_trans;
    hipLaunchKernelGGL(tsdfk::track_solve, dim3(1), dim3(256), 0, v->stream, q);
    HIP_TRY(hipGetLastError());
    return TSDF_OK;
}

// The rule's starting matrix: float32 multiply_matrix(base2world_inv, [first three rows of velo2world; 0 0 0 1]).
void scan_track_start(const tsdf_volume *v, const float velo2world[16], float start[16])
{
    float g[16] = {0};
    std::memcpy(g, velo2world, 12 * sizeof(float));
    g[15] = 1.0f;
    tsdf_host::multiply_matrix(v->base2world_inv, g, start);
}

// The scan in HBM, the state from `velo2world`, the iterations `queue` asks for, and the state back on the host.
template <typename Queue>
int scan_track_run(tsdf_volume *v, const ScanTrackScratch &sc, const float *points_host, const uint8_t *flags_host, int64_t n_points,
                   const float velo2world[16], Queue queue)
{
    int rc = scan_track_upload(v, points_host, flags_host, n_points);
    if (rc) return rc;
    float start[16];
    scan_track_start(v, velo2world, start);
    double M[12];
    for (int i = 0; i < 12; ++i) M[i] = (double)start[i];
    hipLaunchKernelGGL(tsdfk::track_init, dim3(1), dim3(64), 0, v->stream, sc.state, track_initial(M));
    HIP_TRY(hipGetLastError());
    rc = queue();
    if (n_points > 0) HIP_TRY(hipEventRecord(v->scan.pts_read, v->stream));     // behind the last kernel that read the points
    if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(v->h_scan_track.get(), sc.state, sizeof(tsdfk::TrackState), hipMemcpyDeviceToHost, v->stream));
    HIP_TRY(hipStreamSynchronize(v->stream));
    return TSDF_OK;
}

}  // namespace

extern "C" {

int tsdf_scan_track_params_default(const tsdf_config *cfg, tsdf_scan_track_params *out)
{
    if (!cfg || !out) return fail(TSDF_ERR_INVALID, "tsdf_scan_track_params_default: NULL argument");
    // choices, not measurements
    out->weight_thresh = 0.9f;
    out->resid_thresh = cfg->trunc_margin;   // the whole band
    out->min_range_m = 2.5f;                 // the ground rule's min_range: nearer returns are the vehicle's own
    out->max_range_m = 80.0f;
    out->n_levels = 3;
    out->iters[0] = 10; out->iters[1] = 5; out->iters[2] = 4;     // tsdf_track's schedule
    out->min_pairs = 300;                    // tsdf_track's figure
    out->drop_flag = -1;
    out->eps_rot = 1e-5f;
    out->eps_trans = 1e-5f;
    return TSDF_OK;
}

int tsdf_scan_pose(const float R_rect[9], const float R_velo[9], const float t_velo[3], float velo2cam_out[16])
{
    if (!R_rect || !R_velo || !t_velo || !velo2cam_out) return fail(TSDF_ERR_INVALID, "tsdf_scan_pose: NULL argument");
    // tsdf_scan_projection's product without P_rect: [R_rect 0; 0 1] * [R_velo t_velo; 0 1], each entry a left-to-right sum
    float a[16] = {0}, b[16] = {0};
    for (int r = 0; r < 3; ++r) {
        for (int c = 0; c < 3; ++c) { a[4 * r + c] = R_rect[3 * r + c]; b[4 * r + c] = R_velo[3 * r + c]; }
        b[4 * r + 3] = t_velo[r];
    }
    a[15] = b[15] = 1.0f;
    tsdf_host::multiply_matrix(a, b, velo2cam_out);
    return TSDF_OK;
}

int tsdf_scan_track(tsdf_volume *v, const tsdf_scan_track_params *p, const float *points_host, int64_t n_points,
                    const uint8_t *flags_host, const float guess_velo2world[16], tsdf_scan_track_result *out)
{
    const char *who = "tsdf_scan_track";
    int rc = scan_track_checks(who, v, p, points_host, n_points, "guess_velo2world", guess_velo2world, out);
    if (rc) return rc;
    ScanTrackScratch sc;
    rc = scan_track_scratch(v, &sc);
    if (rc) return rc;
    const uint8_t *flags = p->drop_flag >= 0 ? flags_host : nullptr;      // (a byte never equals -1)
    rc = scan_track_run(v, sc, points_host, flags, n_points, guess_velo2world, [&]() {
        int r = TSDF_OK;
        for (int l = p->n_levels - 1; l >= 0 && r == TSDF_OK; --l)
            for (int it = 0; it < p->iters[l] && r == TSDF_OK; ++it)
                r = scan_track_iteration(v, p, sc, n_points, flags != nullptr, l, false);
        return r;
    });
    if (rc) return rc;
    const tsdfk::TrackState &st = *v->h_scan_track.get();
    std::memset(out, 0, sizeof *out);
    for (int l = 0; l < 3; ++l) out->iters_run[l] = st.iters_run[l];
    out->pairs = st.inliers;
    out->rmse = st.inliers > 0 ? (float)std::sqrt(st.r2 / (double)st.inliers) : 0.0f;
    if (st.lost) {                         // the guess's own bits, all 16
        out->status = 2;
        std::memcpy(out->velo2world, guess_velo2world, sizeof out->velo2world);
        return TSDF_OK;
    }
    int last = -1;                         // the finest level that ran
    for (int l = p->n_levels - 1; l >= 0; --l)
        if (p->iters[l] > 0) last = l;
    out->status = last >= 0 && st.done[last] ? 0 : 1;
    // velo2world = base2world * [M; 0 0 0 1], double, sums over k left to right
    const float *bw = v->cfg.base2world;
    double M4[16] = {};
    for (int k = 0; k < 12; ++k) M4[k] = st.M[k];
    M4[15] = 1.0;
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 4; ++j) {
            double acc = (double)bw[4 * i] * M4[j];
            for (int k = 1; k < 4; ++k) acc = acc + (double)bw[4 * i + k] * M4[4 * k + j];
            out->velo2world[4 * i + j] = (float)acc;
        }
    out->velo2world[15] = 1.0f;            // (the memset left 0 0 0 in front of it)
    return TSDF_OK;
}

int tsdf_scan_track_system(tsdf_volume *v, const tsdf_scan_track_params *p, const float *points_host, int64_t n_points,
                           const uint8_t *flags_host, const float velo2world[16], int32_t level, double system_out[29])
{
    const char *who = "tsdf_scan_track_system";
    if (p && p->n_levels >= 1 && p->n_levels <= 3 && (level < 0 || level >= p->n_levels))
        return fail(TSDF_ERR_INVALID, "%s: level %d is outside [0, n_levels = %d)", who, level, p->n_levels);
    int rc = scan_track_checks(who, v, p, points_host, n_points, "velo2world", velo2world, system_out);
    if (rc) return rc;
    ScanTrackScratch sc;
    rc = scan_track_scratch(v, &sc);
    if (rc) return rc;
    const uint8_t *flags = p->drop_flag >= 0 ? flags_host : nullptr;
    rc = scan_track_run(v, sc, points_host, flags, n_points, velo2world,
                        [&]() { return scan_track_iteration(v, p, sc, n_points, flags != nullptr, level, true); });
    if (rc) return rc;
    std::memcpy(system_out, v->h_scan_track.get()->sys, sizeof(double) * tsdfk::kTrackTerms);
    return TSDF_OK;
}

}  // extern "C"
