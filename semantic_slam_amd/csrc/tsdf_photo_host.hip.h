// tsdf_photo_host.hip.h -- host side of photometric tracking (include/tsdf_hip.h: tsdf_track_rgbd*, tsdf_render_intensity),
// included at the end of tsdf_capi.hip after tsdf_track_host.hip.h, whose render, state and geometric pass it uses;
// tsdf_photo.hip.h states the rule.  Every entry point takes host images and returns when its result is on the host, so the
// one pinned staging block of the handle is free again whenever a call begins.
#pragma once

namespace {

int photo_params_ok(const char *who, const tsdf_photo_params *pp)
{
    if (!pp) return fail(TSDF_ERR_INVALID, "%s: NULL photometric parameters", who);
    if (!(std::isfinite(pp->photo_weight) && pp->photo_weight >= 0.0f))
        return fail(TSDF_ERR_INVALID, "%s: photo_weight must be finite and >= 0 (%g)", who, (double)pp->photo_weight);
    if (!(std::isfinite(pp->intensity_thresh) && pp->intensity_thresh > 0.0f))
        return fail(TSDF_ERR_INVALID, "%s: intensity_thresh must be finite and > 0 (%g)", who, (double)pp->intensity_thresh);
    return TSDF_OK;
}

// The handle's photometric block in HBM (grown with the image): the staged frame (depth | rgb | mask), both pyramids, the
// photometric partial rows and state; and its pinned mirror (depth | rgb | mask | state).
struct PhotoScratch {
    float *depth;
    uint8_t *rgb, *mask;
    float *live[tsdfk::kPhotoLevels], *model[tsdfk::kPhotoLevels];
    int w[tsdfk::kPhotoLevels], h[tsdfk::kPhotoLevels];
    double *partials;
    tsdfk::PhotoState *state;
    float *h_depth;
    uint8_t *h_rgb, *h_mask;
    tsdfk::PhotoState *h_state;
};

int photo_scratch(tsdf_volume *v, const tsdf_raycast_params *ray, PhotoScratch *sc)
{
    const size_t px = (size_t)ray->im_height * ray->im_width;
    tsdf_host::Regions r, hr;
    const size_t o_d = r.add(px * 4), o_c = r.add(px * 3), o_m = r.add(px);
    size_t o_live[tsdfk::kPhotoLevels], o_model[tsdfk::kPhotoLevels];
    for (int l = 0; l < tsdfk::kPhotoLevels; ++l) {
        sc->w[l] = ray->im_width >> l;
        sc->h[l] = ray->im_height >> l;
        const size_t n = std::max<size_t>(1, (size_t)sc->w[l] * sc->h[l]);
        o_live[l] = r.add(n * 4);
        o_model[l] = r.add(n * 4);
    }
    const size_t o_p = r.add(sizeof(double) * tsdfk::kTrackMaxBlocks * tsdfk::kTrackTerms);
    const size_t o_s = r.add(sizeof(tsdfk::PhotoState));
    const size_t h_d = hr.add(px * 4), h_c = hr.add(px * 3), h_m = hr.add(px), h_s = hr.add(sizeof(tsdfk::PhotoState));
    HIP_TRY(v->d_photo.ensure(r.total()));
    HIP_TRY(v->h_photo.ensure(hr.total()));
    char *base = v->d_photo, *hb = v->h_photo;
    sc->depth = reinterpret_cast<float *>(base + o_d);
    sc->rgb = reinterpret_cast<uint8_t *>(base + o_c);
    sc->mask = reinterpret_cast<uint8_t *>(base + o_m);
    for (int l = 0; l < tsdfk::kPhotoLevels; ++l) {
        sc->live[l] = reinterpret_cast<float *>(base + o_live[l]);
        sc->model[l] = reinterpret_cast<float *>(base + o_model[l]);
    }
    sc->partials = reinterpret_cast<double *>(base + o_p);
    sc->state = reinterpret_cast<tsdfk::PhotoState *>(base + o_s);
    sc->h_depth = reinterpret_cast<float *>(hb + h_d);
    sc->h_rgb = reinterpret_cast<uint8_t *>(hb + h_c);
    sc->h_mask = reinterpret_cast<uint8_t *>(hb + h_m);
    sc->h_state = reinterpret_cast<tsdfk::PhotoState *>(hb + h_s);
    return TSDF_OK;
}

dim3 photo_flat_grid(size_t n) { return dim3((unsigned)std::max<size_t>(1, (n + 255) / 256)); }

// Levels 1.. of a pyramid from its level 0.
int photo_pyramid(tsdf_volume *v, const PhotoScratch &sc, float *const levels[tsdfk::kPhotoLevels], int n_levels)
{
    for (int l = 1; l < n_levels; ++l) {
        const size_t n = (size_t)sc.w[l] * sc.h[l];
        if (n == 0) break;
        hipLaunchKernelGGL(tsdfk::photo_halve, photo_flat_grid(n), dim3(256), 0, v->stream, levels[l - 1], levels[l], sc.w[l - 1],
                           sc.w[l], sc.h[l]);
        HIP_TRY(hipGetLastError());
    }
    return TSDF_OK;
}

// The host frame into the handle's block (one copy per image through the pinned mirror), queued on the handle's stream; with
// an rgb image, the live pyramid.
int photo_stage(tsdf_volume *v, const tsdf_raycast_params *ray, const PhotoScratch &sc, const float *depth_host,
                const uint8_t *rgb_host, const uint8_t *mask_host, int n_levels)
{
    const size_t px = (size_t)ray->im_height * ray->im_width;
    tsdf_host::copy_to_pinned(sc.h_depth, depth_host, px * 4);
    HIP_TRY(hipMemcpyAsync(sc.depth, sc.h_depth, px * 4, hipMemcpyHostToDevice, v->stream));
    if (mask_host) {
        std::memcpy(sc.h_mask, mask_host, px);
        HIP_TRY(hipMemcpyAsync(sc.mask, sc.h_mask, px, hipMemcpyHostToDevice, v->stream));
    }
    if (rgb_host) {
        std::memcpy(sc.h_rgb, rgb_host, px * 3);
        HIP_TRY(hipMemcpyAsync(sc.rgb, sc.h_rgb, px * 3, hipMemcpyHostToDevice, v->stream));
        hipLaunchKernelGGL(tsdfk::photo_luma, photo_flat_grid(px), dim3(256), 0, v->stream, sc.rgb, sc.live[0], (int)px);
        HIP_TRY(hipGetLastError());
        return photo_pyramid(v, sc, sc.live, n_levels);
    }
    return TSDF_OK;
}

// The model pyramid from the depth render at cam2world (already queued on the handle's stream).
int photo_model(tsdf_volume *v, const tsdf_raycast_params *ray, const PhotoScratch &sc, const float *render_depth,
                const float cam2world[16], int n_levels)
{
    float c2b[16];
    compose_cam2base(v, cam2world, c2b);
    tsdfk::PhotoModelParams k;
    k.vol = ray_volume(v, c2b);
    k.colour = v->d_colour;
    k.depth = render_depth;
    k.out = sc.model[0];
    ray_camera(k, ray);
    hipLaunchKernelGGL(tsdfk::photo_model_intensity, photo_flat_grid((size_t)k.H * k.W), dim3(256), 0, v->stream, k);
    HIP_TRY(hipGetLastError());
    return photo_pyramid(v, sc, sc.model, n_levels);
}

// One combined iteration of level l: the geometric pass (track_pairs, unchanged), the photometric pass and photo_solve.
int photo_iteration(tsdf_volume *v, const tsdf_track_params *p, const tsdf_photo_params *pp, const TrackScratch &ts,
                    const PhotoScratch &sc, bool masked, int level, bool system_only)
{
    const uint8_t *mask = masked ? sc.mask : nullptr;
    const tsdfk::TrackPairsParams g = track_pairs_params(p, ts.depth, ts.normal, sc.depth, mask, ts.state, ts.partials, level);
    const int64_t n = (int64_t)g.ni * g.nj;
    const int nb = (int)std::max<int64_t>(1, std::min<int64_t>((n + 255) / 256, tsdfk::kTrackMaxBlocks));
    hipLaunchKernelGGL(tsdfk::track_pairs, dim3(nb), dim3(256), 0, v->stream, g);
    HIP_TRY(hipGetLastError());
    tsdfk::PhotoPairsParams k;
    k.depth = sc.depth; k.mask = mask; k.live = sc.live[level]; k.model = sc.model[level]; k.model_depth = ts.depth;
    k.state = ts.state; k.partials = sc.partials;
    k.fx = g.fx; k.fy = g.fy; k.cx = g.cx; k.cy = g.cy; k.near_m = g.near_m; k.far_m = g.far_m;
    k.dist = p->dist_thresh[level]; k.ithr = pp->intensity_thresh;
    k.H = g.H; k.W = g.W; k.Hl = sc.h[level]; k.Wl = sc.w[level]; k.s = g.s; k.ni = g.ni; k.nj = g.nj; k.level = level;
    hipLaunchKernelGGL(tsdfk::photo_pairs, dim3(nb), dim3(256), 0, v->stream, k);
    HIP_TRY(hipGetLastError());
    tsdfk::PhotoSolveParams q;
    q.state = ts.state; q.photo = sc.state; q.geo_partials = ts.partials; q.photo_partials = sc.partials;
    q.geo_rows = nb; q.photo_rows = nb; q.level = level; q.min_inliers = p->min_inliers; q.system_only = system_only ? 1 : 0;
    q.lam2 = (double)pp->photo_weight * (double)pp->photo_weight;
    q.eps_rot = p->eps_rot; q.eps_trans = p->eps_trans;
    hipLaunchKernelGGL(tsdfk::photo_solve, dim3(1), dim3(256), 0, v->stream, q);
    HIP_TRY(hipGetLastError());
    return TSDF_OK;
}

// Both states to the host; the handle's stream is waited for whatever rc says, so that the pinned block is free again.
int photo_fetch(tsdf_volume *v, const TrackScratch &ts, const PhotoScratch &sc, int rc)
{
    hipError_t e = hipSuccess;
    if (rc == TSDF_OK) e = hipMemcpyAsync(v->h_track.get(), ts.state, sizeof(tsdfk::TrackState), hipMemcpyDeviceToHost, v->stream);
    if (rc == TSDF_OK && e == hipSuccess)
        e = hipMemcpyAsync(sc.h_state, sc.state, sizeof(tsdfk::PhotoState), hipMemcpyDeviceToHost, v->stream);
    const hipError_t w = hipStreamSynchronize(v->stream);
    if (rc) return rc;
    HIP_TRY(e);
    HIP_TRY(w);
    return TSDF_OK;
}

int photo_checks(const char *who, tsdf_volume *v, const tsdf_track_params *p, const tsdf_photo_params *pp,
                 const float *depth_host, const uint8_t *rgb_host, const float *pose, const void *out)
{
    if (!v || !pose) return fail(TSDF_ERR_INVALID, "%s: NULL argument", who);
    if (!depth_host) return fail(TSDF_ERR_INVALID, "%s: NULL depth frame", who);
    if (!out) return fail(TSDF_ERR_INVALID, "%s: NULL result", who);
    int rc = photo_params_ok(who, pp);
    if (rc) return rc;
    if (rgb_host && !v->d_colour) return fail(TSDF_ERR_INVALID, "%s: an rgb image needs tsdf_colour_enable", who);
    return track_checks(who, v, p, depth_host, pose, out);
}

}  // namespace

extern "C" {

int tsdf_photo_params_default(const tsdf_config *cfg, tsdf_photo_params *out)
{
    if (!cfg || !out) return fail(TSDF_ERR_INVALID, "tsdf_photo_params_default: NULL argument");
    out->photo_weight = 0.1f;       // the weight experiment
    out->intensity_thresh = 0.25f;
    return TSDF_OK;
}

int tsdf_track_rgbd(tsdf_volume *v, const tsdf_track_params *p, const tsdf_photo_params *pp, const float *depth_host,
                    const uint8_t *rgb_host, const uint8_t *mask_host, const float guess_cam2world[16],
                    tsdf_track_rgbd_result *out)
{
    const char *who = "tsdf_track_rgbd";
    int rc = photo_checks(who, v, p, pp, depth_host, rgb_host, guess_cam2world, out);
    if (rc) return rc;
    const bool photo = rgb_host && pp->photo_weight != 0.0f;
    TrackScratch ts;
    PhotoScratch sc;
    rc = track_scratch(v, p, &ts);
    if (rc == TSDF_OK) rc = photo_scratch(v, &p->ray, &sc);
    if (rc) return rc;
    const double eye[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
    rc = photo_stage(v, &p->ray, sc, depth_host, photo ? rgb_host : nullptr, mask_host, p->n_levels);
    if (rc == TSDF_OK) rc = track_begin(v, p, ts, guess_cam2world, eye);
    if (rc == TSDF_OK) {
        hipLaunchKernelGGL(tsdfk::photo_init, dim3(1), dim3(64), 0, v->stream, sc.state);
        if (hipGetLastError() != hipSuccess) rc = fail(TSDF_ERR_HIP, "%s: photo_init failed to launch", who);
    }
    if (rc == TSDF_OK && photo) rc = photo_model(v, &p->ray, sc, ts.depth, guess_cam2world, p->n_levels);
    const uint8_t *mask_dev = mask_host ? sc.mask : nullptr;
    for (int l = p->n_levels - 1; l >= 0 && rc == TSDF_OK; --l)
        for (int it = 0; it < p->iters[l] && rc == TSDF_OK; ++it)
            rc = photo ? photo_iteration(v, p, pp, ts, sc, mask_host != nullptr, l, false)
                       : track_iteration(v->stream, p, ts, sc.depth, mask_dev, l, false);
    rc = photo_fetch(v, ts, sc, rc);
    if (rc) return rc;
    const tsdfk::TrackState &st = *v->h_track.get();
    float cr[16];
    compose_cam2base(v, guess_cam2world, cr);
    const float *bw = v->cfg.base2world;
    double X[16];      // X = base2world * C_ref, double, sums over k left to right
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) {
            double acc = (double)bw[4 * i] * (double)cr[j];
            for (int k = 1; k < 4; ++k) acc = acc + (double)bw[4 * i + k] * (double)cr[4 * k + j];
            X[4 * i + j] = acc;
        }
    track_result(p, st, guess_cam2world, X, &out->geo);
    out->photo_pairs = sc.h_state->pairs;
    out->photo_rmse = sc.h_state->pairs > 0 ? (float)std::sqrt(sc.h_state->r2 / (double)sc.h_state->pairs) : 0.0f;
    return TSDF_OK;
}

int tsdf_track_rgbd_system(tsdf_volume *v, const tsdf_track_params *p, const tsdf_photo_params *pp, const float *depth_host,
                           const uint8_t *rgb_host, const uint8_t *mask_host, const float ref_cam2world[16],
                           const float cam2world[16], int32_t level, double geo_out[29], double photo_out[29])
{
    const char *who = "tsdf_track_rgbd_system";
    if (!cam2world || !photo_out || !rgb_host) return fail(TSDF_ERR_INVALID, "%s: NULL argument", who);
    if (p && (level < 0 || level >= p->n_levels))
        return fail(TSDF_ERR_INVALID, "%s: level %d is outside [0, n_levels = %d)", who, level, p->n_levels);
    int rc = photo_checks(who, v, p, pp, depth_host, rgb_host, ref_cam2world, geo_out);
    if (rc) return rc;
    TrackScratch ts;
    PhotoScratch sc;
    rc = track_scratch(v, p, &ts);
    if (rc == TSDF_OK) rc = photo_scratch(v, &p->ray, &sc);
    if (rc) return rc;
    float cr[16], cc[16];
    compose_cam2base(v, ref_cam2world, cr);
    compose_cam2base(v, cam2world, cc);
    double M[12];
    track_relative(cr, cc, M);
    rc = photo_stage(v, &p->ray, sc, depth_host, rgb_host, mask_host, p->n_levels);
    if (rc == TSDF_OK) rc = track_begin(v, p, ts, ref_cam2world, M);
    if (rc == TSDF_OK) {
        hipLaunchKernelGGL(tsdfk::photo_init, dim3(1), dim3(64), 0, v->stream, sc.state);
        if (hipGetLastError() != hipSuccess) rc = fail(TSDF_ERR_HIP, "%s: photo_init failed to launch", who);
    }
    if (rc == TSDF_OK) rc = photo_model(v, &p->ray, sc, ts.depth, ref_cam2world, p->n_levels);
    if (rc == TSDF_OK) rc = photo_iteration(v, p, pp, ts, sc, mask_host != nullptr, level, true);
    rc = photo_fetch(v, ts, sc, rc);
    if (rc) return rc;
    std::memcpy(geo_out, v->h_track.get()->sys, sizeof(double) * tsdfk::kTrackTerms);
    std::memcpy(photo_out, sc.h_state->sys, sizeof(double) * tsdfk::kTrackTerms);
    return TSDF_OK;
}

int tsdf_render_intensity(tsdf_volume *v, const tsdf_raycast_params *p, const float cam2world[16], int32_t level,
                          float *intensity_host)
{
    const char *who = "tsdf_render_intensity";
    if (!intensity_host) return fail(TSDF_ERR_INVALID, "%s: NULL argument", who);
    if (level < 0 || level >= tsdfk::kPhotoLevels)
        return fail(TSDF_ERR_INVALID, "%s: level %d is outside [0, %d)", who, level, tsdfk::kPhotoLevels);
    if (v && v->group_owner)
        return fail(TSDF_ERR_INVALID, "%s: the handle is a slab of a tsdf_group; it needs a whole-grid handle", who);
    int rc = raycast_checks(who, v, p, cam2world, true, false, true);
    if (rc) return rc;
    PhotoScratch sc;
    rc = photo_scratch(v, p, &sc);
    if (rc) return rc;
    const size_t n = (size_t)sc.w[level] * sc.h[level];
    rc = launch_raycast(v, p, cam2world, sc.depth, nullptr, nullptr, nullptr);      // the depth render, in the frame's place
    if (rc == TSDF_OK) rc = photo_model(v, p, sc, sc.depth, cam2world, level + 1);
    hipError_t e = hipSuccess;
    if (rc == TSDF_OK && n > 0) e = hipMemcpyAsync(intensity_host, sc.model[level], n * 4, hipMemcpyDeviceToHost, v->stream);
    const hipError_t w = hipStreamSynchronize(v->stream);
    if (rc) return rc;
    HIP_TRY(e);
    HIP_TRY(w);
    return TSDF_OK;
}

}  // extern "C"
