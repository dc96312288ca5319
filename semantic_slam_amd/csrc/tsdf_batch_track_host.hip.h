// tsdf_batch_track_host.hip.h -- host side of joint tracking against a batch (include/tsdf_hip.h: tsdf_batch_track,
// tsdf_batch_track_system, tsdf_track_member_systems; tsdf_batch_track.hip.h states the rule), included at the end of
// tsdf_capi.hip after tsdf_track_host.hip.h, whose iteration and host arithmetic it uses, and tsdf_associate_host.hip.h.
#pragma once

namespace {

// Workgroups per member tile of a member pass over n samples: track_pairs' count, fewer once members x workgroups partial rows
// would pass kTrackMemberMaxRows.
int member_pass_blocks(int64_t n, int M)
{
    const int64_t cap = std::min<int64_t>(tsdfk::kTrackMaxBlocks, std::max(1, tsdfk::kTrackMemberMaxRows / M));
    return (int)std::max<int64_t>(1, std::min<int64_t>((n + 255) / 256, cap));
}

// The result block (state | member systems) is one region on the device and one in pinned memory: one copy brings both.
size_t member_systems_offset() { return (sizeof(tsdfk::TrackState) + 7) / 8 * 8; }
size_t member_result_bytes(int M) { return member_systems_offset() + sizeof(double) * tsdfk::kTrackTerms * (size_t)M; }

struct BatchTrackScratch {
    float *depth, *normal, *joint;     // the render; its depth with the members that are out zeroed
    int32_t *member;
    double *partials, *rows;           // of the joint iterations; of the member pass
    char *result;                      // TrackState | M x 29 doubles
    uint8_t *use;
    char *h_result;                    // pinned: the result block, then M bytes of member_use
    uint8_t *h_use;
};

int batch_track_scratch(tsdf_batch *b, const tsdf_track_params *p, BatchTrackScratch *sc)
{
    const int M = (int)b->vols.size();
    const size_t px = (size_t)p->ray.im_height * p->ray.im_width;
    const int nb = member_pass_blocks((int64_t)px, M);       // level 0 has the most samples, fewer than px
    tsdf_host::Regions r;
    const size_t o_d = r.add(px * 4), o_n = r.add(px * 12), o_j = r.add(px * 4), o_m = r.add(px * 4);
    const size_t o_p = r.add(sizeof(double) * tsdfk::kTrackMaxBlocks * tsdfk::kTrackTerms);
    const size_t o_r = r.add(sizeof(double) * tsdfk::kTrackTerms * (size_t)M * nb);
    const size_t o_s = r.add(member_result_bytes(M)), o_u = r.add((size_t)M);
    HIP_TRY(b->d_track.ensure(r.total()));
    HIP_TRY(b->h_track.ensure(member_result_bytes(M) + (size_t)M));
    char *base = b->d_track;
    sc->depth = reinterpret_cast<float *>(base + o_d);
    sc->normal = reinterpret_cast<float *>(base + o_n);
    sc->joint = reinterpret_cast<float *>(base + o_j);
    sc->member = reinterpret_cast<int32_t *>(base + o_m);
    sc->partials = reinterpret_cast<double *>(base + o_p);
    sc->rows = reinterpret_cast<double *>(base + o_r);
    sc->result = base + o_s;
    sc->use = reinterpret_cast<uint8_t *>(base + o_u);
    sc->h_result = b->h_track.get();
    sc->h_use = reinterpret_cast<uint8_t *>(sc->h_result + member_result_bytes(M));
    return TSDF_OK;
}

// The member pass of level `level` at the state's pose, queued on s: S[m] of every member into `systems`.
int launch_member_pass(hipStream_t s, const tsdf_track_params *p, const float *model_depth, const float *model_normal,
                       const int32_t *member, int M, const float *depth_dev, const uint8_t *mask_dev,
                       const tsdfk::TrackState *state, int level, double *rows, double *systems)
{
    tsdfk::TrackMemberParams q;
    q.pp = track_pairs_params(p, model_depth, model_normal, depth_dev, mask_dev, state, nullptr, level);
    q.member = member; q.rows = rows; q.n_members = M;
    const int nb = member_pass_blocks((int64_t)q.pp.ni * q.pp.nj, M);
    const int tiles = (M + tsdfk::kTrackMemberTile - 1) / tsdfk::kTrackMemberTile;
    hipLaunchKernelGGL(tsdfk::track_member_pairs, dim3(nb, tiles), dim3(256), 0, s, q);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(tsdfk::track_member_sum, dim3(M), dim3(256), 0, s, state, rows, nb, systems);
    HIP_TRY(hipGetLastError());
    return TSDF_OK;
}

int batch_track_checks(const char *who, tsdf_batch *b, const tsdf_track_params *p, const float *depth_dev,
                       const float *pose_a, const float *pose_b, const void *out, int32_t level)
{
    if (!b || !pose_a || !pose_b) return fail(TSDF_ERR_INVALID, "%s: NULL argument", who);
    if (!depth_dev) return fail(TSDF_ERR_INVALID, "%s: NULL depth frame", who);
    if (!out) return fail(TSDF_ERR_INVALID, "%s: NULL result", who);
    int rc = track_params_ok(who, p);
    if (rc) return rc;
    if (level < 0 || level >= p->n_levels)
        return fail(TSDF_ERR_INVALID, "%s: level %d is outside [0, n_levels = %d)", who, level, p->n_levels);
    rc = assoc_sizes_ok(who, 1, (int)b->vols.size());
    if (rc) return rc;
    const tsdf_config &c0 = b->vols[0]->cfg;
    if (p->ray.im_height != c0.im_height || p->ray.im_width != c0.im_width)
        return fail(TSDF_ERR_INVALID, "%s: the render is %dx%d, the batch's frames %dx%d", who, p->ray.im_width,
                    p->ray.im_height, c0.im_width, c0.im_height);
    return batch_render_checks(who, b, &p->ray);   // a z-slab member is refused; then the collected frames
}

}  // namespace

extern "C" {

int tsdf_batch_track(tsdf_batch *b, const tsdf_track_params *p, const float *depth_dev, const uint8_t *mask_dev,
                     const uint8_t *member_use, const float guess_cam2world[16], tsdf_track_result *out,
                     double *member_systems)
{
    const char *who = "tsdf_batch_track";
    int rc = batch_track_checks(who, b, p, depth_dev, guess_cam2world, guess_cam2world, out, 0);
    if (rc) return rc;
    const int M = (int)b->vols.size();
    BatchTrackScratch sc;
    rc = batch_track_scratch(b, p, &sc);
    if (rc) return rc;
    hipStream_t s = b->stream;
    for (int m = 0; m < M; ++m) sc.h_use[m] = member_use ? (member_use[m] != 0) : 1;
    HIP_TRY(hipMemcpyAsync(sc.use, sc.h_use, (size_t)M, hipMemcpyHostToDevice, s));
    rc = batch_render(b, &p->ray, guess_cam2world, sc.depth, sc.normal, sc.member);
    if (rc) return rc;
    const int64_t px = (int64_t)p->ray.im_height * p->ray.im_width;
    const int nbm = (int)std::min<int64_t>((px + 255) / 256, 1024);
    hipLaunchKernelGGL(tsdfk::track_mask_model, dim3(nbm), dim3(256), 0, s, sc.depth, sc.member, sc.use, M, sc.joint, px);
    HIP_TRY(hipGetLastError());
    tsdfk::TrackState *state = reinterpret_cast<tsdfk::TrackState *>(sc.result);
    double *systems = reinterpret_cast<double *>(sc.result + member_systems_offset());
    const double eye[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
    hipLaunchKernelGGL(tsdfk::track_init, dim3(1), dim3(64), 0, s, state, track_initial(eye));
    HIP_TRY(hipGetLastError());
    const TrackScratch joint = {sc.joint, sc.normal, sc.partials, state};
    int last = -1;                         // the finest level that runs
    for (int l = p->n_levels - 1; l >= 0 && rc == TSDF_OK; --l) {
        if (p->iters[l] > 0) last = l;
        for (int it = 0; it < p->iters[l] && rc == TSDF_OK; ++it) rc = track_iteration(s, p, joint, depth_dev, mask_dev, l, false);
    }
    if (rc == TSDF_OK && member_systems)       // nobody reads the member pass of a caller that wants the pose alone
        rc = launch_member_pass(s, p, sc.depth, sc.normal, sc.member, M, depth_dev, mask_dev, state, last < 0 ? 0 : last,
                                sc.rows, systems);
    if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(sc.h_result, sc.result, member_systems ? member_result_bytes(M) : sizeof(tsdfk::TrackState),
                           hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    const tsdfk::TrackState &st = *reinterpret_cast<const tsdfk::TrackState *>(sc.h_result);
    if (member_systems)
        std::memcpy(member_systems, sc.h_result + member_systems_offset(), sizeof(double) * tsdfk::kTrackTerms * (size_t)M);
    double X[16];                          // C_ref itself: the rule works in the reference camera's frame
    for (int k = 0; k < 16; ++k) X[k] = (double)guess_cam2world[k];
    track_result(p, st, guess_cam2world, X, out);
    return TSDF_OK;
}

int tsdf_batch_track_system(tsdf_batch *b, const tsdf_track_params *p, const float *depth_dev, const uint8_t *mask_dev,
                            const float ref_cam2world[16], const float cam2world[16], int32_t level, double *member_systems)
{
    const char *who = "tsdf_batch_track_system";
    int rc = batch_track_checks(who, b, p, depth_dev, ref_cam2world, cam2world, member_systems, level);
    if (rc) return rc;
    const int M = (int)b->vols.size();
    BatchTrackScratch sc;
    rc = batch_track_scratch(b, p, &sc);
    if (rc) return rc;
    hipStream_t s = b->stream;
    rc = batch_render(b, &p->ray, ref_cam2world, sc.depth, sc.normal, sc.member);
    if (rc) return rc;
    double Mrel[12];
    track_relative(ref_cam2world, cam2world, Mrel);
    tsdfk::TrackState *state = reinterpret_cast<tsdfk::TrackState *>(sc.result);
    double *systems = reinterpret_cast<double *>(sc.result + member_systems_offset());
    hipLaunchKernelGGL(tsdfk::track_init, dim3(1), dim3(64), 0, s, state, track_initial(Mrel));
    HIP_TRY(hipGetLastError());
    rc = launch_member_pass(s, p, sc.depth, sc.normal, sc.member, M, depth_dev, mask_dev, state, level, sc.rows, systems);
    if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(sc.h_result, sc.result, member_result_bytes(M), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    std::memcpy(member_systems, sc.h_result + member_systems_offset(), sizeof(double) * tsdfk::kTrackTerms * (size_t)M);
    return TSDF_OK;
}

int tsdf_track_member_systems(int32_t device, const tsdf_track_params *p, const float *model_depth_dev,
                              const float *model_normal_dev, const int32_t *member_dev, int32_t n_members,
                              const float *depth_dev, const uint8_t *mask_dev, const float ref_cam2world[16],
                              const float cam2world[16], int32_t level, double *member_systems)
{
    const char *who = "tsdf_track_member_systems";
    if (!model_depth_dev || !model_normal_dev || !member_dev || !depth_dev || !ref_cam2world || !cam2world || !member_systems)
        return fail(TSDF_ERR_INVALID, "%s: NULL argument", who);
    int rc = track_params_ok(who, p);
    if (rc) return rc;
    if (level < 0 || level >= p->n_levels)
        return fail(TSDF_ERR_INVALID, "%s: level %d is outside [0, n_levels = %d)", who, level, p->n_levels);
    rc = assoc_sizes_ok(who, 1, n_members);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(device));
    // the images may have been produced on a handle's (non-blocking) stream, which the null stream does not order against
    HIP_TRY(hipDeviceSynchronize());
    const int64_t px = (int64_t)p->ray.im_height * p->ray.im_width;
    const int nb = member_pass_blocks(px, n_members);
    tsdf_host::Regions r;
    const size_t o_r = r.add(sizeof(double) * tsdfk::kTrackTerms * (size_t)n_members * nb);
    const size_t o_s = r.add(sizeof(tsdfk::TrackState));
    const size_t o_y = r.add(sizeof(double) * tsdfk::kTrackTerms * (size_t)n_members);
    DevPtr<char> block;
    HIP_TRY(dev_alloc(block, r.total()));
    char *base = block;
    tsdfk::TrackState *state = reinterpret_cast<tsdfk::TrackState *>(base + o_s);
    double *systems = reinterpret_cast<double *>(base + o_y);
    double Mrel[12];
    track_relative(ref_cam2world, cam2world, Mrel);
    hipLaunchKernelGGL(tsdfk::track_init, dim3(1), dim3(64), 0, 0, state, track_initial(Mrel));
    HIP_TRY(hipGetLastError());
    rc = launch_member_pass(0, p, model_depth_dev, model_normal_dev, member_dev, n_members, depth_dev, mask_dev, state, level,
                            reinterpret_cast<double *>(base + o_r), systems);
    if (rc) return rc;
    HIP_TRY(hipMemcpy(member_systems, systems, sizeof(double) * tsdfk::kTrackTerms * (size_t)n_members, hipMemcpyDeviceToHost));
    return TSDF_OK;
}

}  // extern "C"
