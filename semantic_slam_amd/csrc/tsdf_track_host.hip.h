// tsdf_track_host.hip.h -- host side of tracking (include/tsdf_hip.h: tsdf_track*), included at the end of tsdf_capi.hip after
// tsdf_raycast_host.hip.h, whose render it uses; tsdf_track.hip.h states the rule.
#pragma once

namespace {

int track_params_ok(const char *who, const tsdf_track_params *p)
{
    if (!p) return fail(TSDF_ERR_INVALID, "%s: NULL parameters", who);
    int rc = ray_params_ok(who, &p->ray);
    if (rc) return rc;
    if (p->n_levels < 1 || p->n_levels > 3) return fail(TSDF_ERR_INVALID, "%s: n_levels %d is outside 1..3", who, p->n_levels);
    for (int l = 0; l < p->n_levels; ++l) {
        if (p->iters[l] < 0) return fail(TSDF_ERR_INVALID, "%s: iters[%d] = %d is negative", who, l, p->iters[l]);
        if (!(std::isfinite(p->dist_thresh[l]) && p->dist_thresh[l] > 0.0f))
            return fail(TSDF_ERR_INVALID, "%s: dist_thresh[%d] must be finite and > 0 (%g)", who, l, (double)p->dist_thresh[l]);
    }
    if (!(p->cos_normal_thresh >= -1.0f && p->cos_normal_thresh <= 1.0f))
        return fail(TSDF_ERR_INVALID, "%s: cos_normal_thresh must lie in [-1, 1] (%g)", who, (double)p->cos_normal_thresh);
    if (p->min_inliers < 0) return fail(TSDF_ERR_INVALID, "%s: min_inliers %d is negative", who, p->min_inliers);
    if (!(std::isfinite(p->eps_rot) && p->eps_rot > 0.0f && std::isfinite(p->eps_trans) && p->eps_trans > 0.0f))
        return fail(TSDF_ERR_INVALID, "%s: eps_rot and eps_trans must be finite and > 0 (%g, %g)", who, (double)p->eps_rot,
                    (double)p->eps_trans);
    return TSDF_OK;
}

int track_checks(const char *who, tsdf_volume *v, const tsdf_track_params *p, const float *depth_dev,
                        const float *pose, const void *out)
{
    if (!v || !pose) return fail(TSDF_ERR_INVALID, "%s: NULL argument", who);
    if (!depth_dev) return fail(TSDF_ERR_INVALID, "%s: NULL depth frame", who);
    if (!out) return fail(TSDF_ERR_INVALID, "%s: NULL result", who);
    int rc = track_params_ok(who, p);
    if (rc == TSDF_OK) rc = ray_volume_ok(who, v);
    if (rc) return rc;
    if (v->group_owner) return fail(TSDF_ERR_INVALID, "%s: the handle is a slab of a tsdf_group; tracking needs a whole-grid handle", who);
    return bind_device(v);   // the collected frames first
}

// The scratch block: model depth | model normal | partial rows | state (kept on the handle, grown with the image).
struct TrackScratch {
    float *depth, *normal;
    double *partials;
    tsdfk::TrackState *state;
};

int track_scratch(tsdf_volume *v, const tsdf_track_params *p, TrackScratch *sc)
{
    const size_t px = (size_t)p->ray.im_height * p->ray.im_width;
    tsdf_host::Regions r;
    const size_t o_d = r.add(px * 4), o_n = r.add(px * 12), o_p = r.add(sizeof(double) * tsdfk::kTrackMaxBlocks * tsdfk::kTrackTerms);
    const size_t o_s = r.add(sizeof(tsdfk::TrackState));
    if (!v->h_track) HIP_TRY(host_alloc(v->h_track, sizeof(tsdfk::TrackState), hipHostMallocDefault));
    HIP_TRY(v->d_track.ensure(r.total()));
    char *base = v->d_track;
    sc->depth = reinterpret_cast<float *>(base + o_d);
    sc->normal = reinterpret_cast<float *>(base + o_n);
    sc->partials = reinterpret_cast<double *>(base + o_p);
    sc->state = reinterpret_cast<tsdfk::TrackState *>(base + o_s);
    return TSDF_OK;
}

// M = C_ref^-1 * C_cur with the rigid inverse, in double from the float32 entries (the rule's "Poses").
void track_relative(const float cr[16], const float cc[16], double M[12])
{
    for (int i = 0; i < 3; ++i) {
        for (int j = 0; j < 3; ++j)
            M[4 * i + j] = ((double)cr[i] * (double)cc[j] + (double)cr[4 + i] * (double)cc[4 + j]) +
                           (double)cr[8 + i] * (double)cc[8 + j];
        M[4 * i + 3] = ((double)cr[i] * ((double)cc[3] - (double)cr[3]) + (double)cr[4 + i] * ((double)cc[7] - (double)cr[7])) +
                       (double)cr[8 + i] * ((double)cc[11] - (double)cr[11]);
    }
}

tsdfk::TrackState track_initial(const double M[12])
{
    tsdfk::TrackState s = {};
    for (int i = 0; i < 3; ++i) {
        for (int j = 0; j < 4; ++j) s.M[4 * i + j] = M[4 * i + j];
        for (int j = 0; j < 3; ++j) s.Rm[3 * i + j] = (float)M[4 * i + j];
        s.tm[i] = (float)M[4 * i + 3];
    }
    return s;
}

// The render at ref_cam2world and the initial state, queued on the handle's stream.
int track_begin(tsdf_volume *v, const tsdf_track_params *p, const TrackScratch &sc, const float ref_cam2world[16],
                       const double M[12])
{
    int rc = launch_raycast(v, &p->ray, ref_cam2world, sc.depth, sc.normal, nullptr, nullptr);
    if (rc) return rc;
    hipLaunchKernelGGL(tsdfk::track_init, dim3(1), dim3(64), 0, v->stream, sc.state, track_initial(M));
    HIP_TRY(hipGetLastError());
    return TSDF_OK;
}

// One association pass of level l as track_pairs (and the member pass of tsdf_batch_track.hip.h) reads it.
tsdfk::TrackPairsParams track_pairs_params(const tsdf_track_params *p, const float *model_depth, const float *model_normal,
                                           const float *depth_dev, const uint8_t *mask_dev, const tsdfk::TrackState *state,
                                           double *partials, int level)
{
    const int s = 1 << level, W = p->ray.im_width, H = p->ray.im_height;
    tsdfk::TrackPairsParams k;
    k.depth = depth_dev; k.mask = mask_dev; k.model_depth = model_depth; k.model_normal = model_normal;
    k.state = state; k.partials = partials;
    k.fx = p->ray.cam_K[0]; k.fy = p->ray.cam_K[4]; k.cx = p->ray.cam_K[2]; k.cy = p->ray.cam_K[5];
    k.near_m = p->ray.near_m; k.far_m = p->ray.far_m;
    k.dist2 = p->dist_thresh[level] * p->dist_thresh[level];
    k.cos_thresh = p->cos_normal_thresh;
    k.H = H; k.W = W; k.s = s; k.level = level;
    k.ni = W > s ? (W - 1 - s) / s + 1 : 0;
    k.nj = H > s ? (H - 1 - s) / s + 1 : 0;
    return k;
}

// One iteration of level l, queued on `stream`: the association pass and the solve (system_only: the summed system, no step).
int track_iteration(hipStream_t stream, const tsdf_track_params *p, const TrackScratch &sc, const float *depth_dev,
                           const uint8_t *mask_dev, int level, bool system_only)
{
    const tsdfk::TrackPairsParams k = track_pairs_params(p, sc.depth, sc.normal, depth_dev, mask_dev, sc.state, sc.partials, level);
    const int64_t n = (int64_t)k.ni * k.nj;
    const int nb = (int)std::max<int64_t>(1, std::min<int64_t>((n + 255) / 256, tsdfk::kTrackMaxBlocks));
    hipLaunchKernelGGL(tsdfk::track_pairs, dim3(nb), dim3(256), 0, stream, k);
    HIP_TRY(hipGetLastError());
    tsdfk::TrackSolveParams q;
    q.state = sc.state; q.partials = sc.partials; q.n_rows = nb; q.level = level; q.min_inliers = p->min_inliers;
    q.system_only = system_only ? 1 : 0;
    q.eps_rot = p->eps_rot; q.eps_trans = p->eps_trans;
    hipLaunchKernelGGL(tsdfk::track_solve, dim3(1), dim3(256), 0, stream, q);
    HIP_TRY(hipGetLastError());
    return TSDF_OK;
}

// The result of a track from its final state: a lost track returns the guess's own bits, any other cam2world = X * M (4 x 4,
// double, sums over k left to right) rounded to float32, with X = base2world * C_ref.
void track_result(const tsdf_track_params *p, const tsdfk::TrackState &st, const float guess_cam2world[16], const double X[16],
                  tsdf_track_result *out)
{
    std::memset(out, 0, sizeof *out);
    for (int l = 0; l < 3; ++l) out->iters_run[l] = st.iters_run[l];
    out->inliers = st.inliers;
    out->rmse = st.inliers > 0 ? (float)std::sqrt(st.r2 / (double)st.inliers) : 0.0f;
    if (st.lost) {
        out->status = 2;
        std::memcpy(out->cam2world, guess_cam2world, sizeof out->cam2world);
        return;
    }
    int last = -1;                         // the finest level that ran
    for (int l = p->n_levels - 1; l >= 0; --l)
        if (p->iters[l] > 0) last = l;
    out->status = last >= 0 && st.done[last] ? 0 : 1;
    double M4[16] = {};
    for (int k = 0; k < 12; ++k) M4[k] = st.M[k];
    M4[15] = 1.0;
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) {
            double acc = X[4 * i] * M4[j];
            for (int k = 1; k < 4; ++k) acc = acc + X[4 * i + k] * M4[4 * k + j];
            out->cam2world[4 * i + j] = (float)acc;
        }
}

int track_fetch(tsdf_volume *v, const TrackScratch &sc)
{
    HIP_TRY(hipMemcpyAsync(v->h_track.get(), sc.state, sizeof(tsdfk::TrackState), hipMemcpyDeviceToHost, v->stream));
    HIP_TRY(hipStreamSynchronize(v->stream));
    return TSDF_OK;
}

}  // namespace

extern "C" {

int tsdf_track_params_default(const tsdf_config *cfg, tsdf_track_params *out)
{
    if (!cfg || !out) return fail(TSDF_ERR_INVALID, "tsdf_track_params_default: NULL argument");
    int rc = tsdf_raycast_params_default(cfg, &out->ray);
    if (rc) return rc;
    out->n_levels = 3;
    out->iters[0] = 10; out->iters[1] = 5; out->iters[2] = 4;
    for (int l = 0; l < 3; ++l) out->dist_thresh[l] = 0.10f;
    out->cos_normal_thresh = (float)std::cos(20.0 * M_PI / 180.0);
    out->min_inliers = 300;
    out->eps_rot = 1e-5f;
    out->eps_trans = 1e-5f;
    return TSDF_OK;
}

int tsdf_track(tsdf_volume *v, const tsdf_track_params *p, const float *depth_dev, const uint8_t *mask_dev,
               const float guess_cam2world[16], tsdf_track_result *out)
{
    const char *who = "tsdf_track";
    int rc = track_checks(who, v, p, depth_dev, guess_cam2world, out);
    if (rc) return rc;
    TrackScratch sc;
    rc = track_scratch(v, p, &sc);
    if (rc) return rc;
    const double eye[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
    rc = track_begin(v, p, sc, guess_cam2world, eye);
    for (int l = p->n_levels - 1; l >= 0 && rc == TSDF_OK; --l)
        for (int it = 0; it < p->iters[l] && rc == TSDF_OK; ++it) rc = track_iteration(v->stream, p, sc, depth_dev, mask_dev, l, false);
    if (rc == TSDF_OK) rc = track_fetch(v, sc);
    if (rc) return rc;
    const tsdfk::TrackState &st = *v->h_track.get();
    // X = base2world * C_ref, double, sums over k left to right
    float cr[16];
    compose_cam2base(v, guess_cam2world, cr);
    const float *bw = v->cfg.base2world;
    double X[16];
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) {
            double acc = (double)bw[4 * i] * (double)cr[j];
            for (int k = 1; k < 4; ++k) acc = acc + (double)bw[4 * i + k] * (double)cr[4 * k + j];
            X[4 * i + j] = acc;
        }
    track_result(p, st, guess_cam2world, X, out);
    return TSDF_OK;
}

int tsdf_track_system(tsdf_volume *v, const tsdf_track_params *p, const float *depth_dev, const uint8_t *mask_dev,
                      const float ref_cam2world[16], const float cam2world[16], int32_t level, double system_out[29])
{
    const char *who = "tsdf_track_system";
    if (!cam2world) return fail(TSDF_ERR_INVALID, "%s: NULL argument", who);
    if (p && (level < 0 || level >= p->n_levels))
        return fail(TSDF_ERR_INVALID, "%s: level %d is outside [0, n_levels = %d)", who, level, p->n_levels);
    int rc = track_checks(who, v, p, depth_dev, ref_cam2world, system_out);
    if (rc) return rc;
    TrackScratch sc;
    rc = track_scratch(v, p, &sc);
    if (rc) return rc;
    float cr[16], cc[16];
    compose_cam2base(v, ref_cam2world, cr);
    compose_cam2base(v, cam2world, cc);
    double M[12];
    track_relative(cr, cc, M);
    rc = track_begin(v, p, sc, ref_cam2world, M);
    if (rc == TSDF_OK) rc = track_iteration(v->stream, p, sc, depth_dev, mask_dev, level, true);
    if (rc == TSDF_OK) rc = track_fetch(v, sc);
    if (rc) return rc;
    std::memcpy(system_out, v->h_track.get()->sys, sizeof(double) * tsdfk::kTrackTerms);
    return TSDF_OK;
}

}  // extern "C"
