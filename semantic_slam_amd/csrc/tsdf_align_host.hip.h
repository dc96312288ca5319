// tsdf_align_host.hip.h -- host side of volume-to-volume registration (include/tsdf_hip.h: tsdf_align_*), included at the end of
// tsdf_capi.hip after tsdf_track_host.hip.h and tsdf_fuse_host.hip.h, whose state, handle checks and event order it uses;
// tsdf_align.hip.h states the rule.
#pragma once

namespace {

int align_params_ok(const char *who, const tsdf_align_params *p)
{
    if (!std::isfinite(p->weight_thresh)) return fail(TSDF_ERR_INVALID, "%s: weight_thresh is not finite", who);
    if (!(std::isfinite(p->resid_thresh) && p->resid_thresh > 0.0f))
        return fail(TSDF_ERR_INVALID, "%s: resid_thresh must be finite and > 0 (%g)", who, (double)p->resid_thresh);
    if (p->n_levels < 1 || p->n_levels > 3) return fail(TSDF_ERR_INVALID, "%s: n_levels %d is outside 1..3", who, p->n_levels);
    for (int l = 0; l < p->n_levels; ++l)
        if (p->iters[l] < 0) return fail(TSDF_ERR_INVALID, "%s: iters[%d] = %d is negative", who, l, p->iters[l]);
    if (p->min_pairs < 0) return fail(TSDF_ERR_INVALID, "%s: min_pairs %d is negative", who, p->min_pairs);
    if (!(std::isfinite(p->eps_rot) && p->eps_rot > 0.0f && std::isfinite(p->eps_trans) && p->eps_trans > 0.0f))
        return fail(TSDF_ERR_INVALID, "%s: eps_rot and eps_trans must be finite and > 0 (%g, %g)", who, (double)p->eps_rot,
                    (double)p->eps_trans);
    return TSDF_OK;
}

// Everything refused before anything is queued; then the collected frames of both handles.
int align_checks(const char *who, tsdf_volume *dst, tsdf_volume *src, const tsdf_align_params *p, const char *pose_name,
                 const float *pose, const void *out)
{
    if (!dst || !src || !p) return fail(TSDF_ERR_INVALID, "%s: NULL argument", who);
    if (!out) return fail(TSDF_ERR_INVALID, "%s: NULL result", who);
    int rc = fuse_pair_ok(who, dst, src);
    if (rc == TSDF_OK) rc = align_params_ok(who, p);
    if (rc) return rc;
    const tsdf_config &cs = src->cfg;
    if (cs.dim_x < 2 || cs.dim_y < 2 || cs.dim_z < 2)
        return fail(TSDF_ERR_INVALID, "%s: every src dim must be >= 2 (%d x %d x %d)", who, cs.dim_x, cs.dim_y, cs.dim_z);
    for (int i = 0; pose && i < 12; ++i)
        if (!std::isfinite(pose[i])) return fail(TSDF_ERR_INVALID, "%s: %s[%d] is not finite", who, pose_name, i);
    rc = bind_device(dst);
    if (rc == TSDF_OK) rc = bind_device(src);
    return rc;
}

// The scratch block on dst: partial rows | state, the state's pinned copy and the two events, all or none; no size of either
// volume enters it.
struct AlignScratch {
    double *partials;
    tsdfk::TrackState *state;
};

int align_scratch(tsdf_volume *dst, AlignScratch *sc)
{
    tsdf_host::Regions r;
    const size_t o_p = r.add(sizeof(double) * tsdfk::kAlignMaxBlocks * tsdfk::kTrackTerms);
    const size_t o_s = r.add(sizeof(tsdfk::TrackState));
    if (!dst->d_align) {
        DevPtr<char> d;
        HostPtr<tsdfk::TrackState> h;
        Event ready, done;
        HIP_TRY(dev_alloc(d, r.total()));
        HIP_TRY(host_alloc(h, sizeof(tsdfk::TrackState), hipHostMallocDefault));
        HIP_TRY(event_create(ready));
        HIP_TRY(event_create(done));
        dst->d_align = std::move(d); dst->h_align = std::move(h);
        dst->align_src_ready = std::move(ready); dst->align_done = std::move(done);
    }
    char *base = dst->d_align;
    sc->partials = reinterpret_cast<double *>(base + o_p);
    sc->state = reinterpret_cast<tsdfk::TrackState *>(base + o_s);
    return TSDF_OK;
}

// One pass of level `level` as align_pairs reads it, and its grid.
tsdfk::AlignPairsParams align_pairs_params(const tsdf_volume *dst, const tsdf_volume *src, const tsdf_align_params *p,
                                           const AlignScratch &sc, int level, int *n_blocks)
{
    const tsdf_config &cd = dst->cfg, &cs = src->cfg;
    const int s = 1 << level;
    tsdfk::AlignPairsParams k;
    k.dt = dst->d_tsdf; k.dw = dst->d_weight;
    k.st = src->d_tsdf; k.sw = src->d_weight;
    k.state = sc.state; k.partials = sc.partials;
    const int sd[3] = {cs.dim_x, cs.dim_y, cs.dim_z}, dd[3] = {cd.dim_x, cd.dim_y, cd.dim_z};
    for (int i = 0; i < 3; ++i) {
        k.od[i] = cd.origin[i]; k.os[i] = cs.origin[i];
        k.hi[i] = (float)(sd[i] - 1);
        k.sdim[i] = sd[i]; k.ddim[i] = dd[i];
        k.ln[i] = (dd[i] + s - 1) / s;
    }
    k.vsd = cd.voxel_size; k.vss = cs.voxel_size;
    k.tiles_x = (k.ln[0] + tsdfk::kAlignTileX - 1) / tsdfk::kAlignTileX;
    k.tiles_y = (k.ln[1] + tsdfk::kAlignTileY - 1) / tsdfk::kAlignTileY;
    const int64_t lanes = (int64_t)k.tiles_x * k.tiles_y * k.ln[2] * 64;
    k.n_lanes = (unsigned)lanes;
    k.s = s; k.level = level;
    k.ratio = cs.trunc_margin / cd.trunc_margin;
    k.gscale = k.ratio / cs.voxel_size;
    k.wthr = p->weight_thresh; k.rthr = p->resid_thresh;
    *n_blocks = (int)std::max<int64_t>(1, std::min<int64_t>((lanes + 255) / 256, tsdfk::kAlignMaxBlocks));
    return k;
}

// One iteration of level `level` on dst's stream: the pair pass and the solve (system_only: the summed system, no step).
int align_iteration(tsdf_volume *dst, tsdf_volume *src, const tsdf_align_params *p, const AlignScratch &sc, int level,
                    bool system_only)
{
    int nb = 0;
    const tsdfk::AlignPairsParams k = align_pairs_params(dst, src, p, sc, level, &nb);
    hipLaunchKernelGGL(tsdfk::align_pairs, dim3(nb), dim3(256), 0, dst->stream, k);
    HIP_TRY(hipGetLastError());
    tsdfk::TrackSolveParams q;
    q.state = sc.state; q.partials = sc.partials; q.n_rows = nb; q.level = level; q.min_inliers = p->min_pairs;
    q.system_only = system_only ? 1 : 0;
    q.eps_rot = p->eps_rot; q.eps_trans = p->eps_trans;
    hipLaunchKernelGGL(tsdfk::track_solve, dim3(1), dim3(256), 0, dst->stream, q);
    HIP_TRY(hipGetLastError());
    return TSDF_OK;
}

// The state from the first three rows of `start`, the iterations `queue` asks for, and the state back on the host: queued on
// dst's stream between the two events of the merge's order.
template <typename Queue>
int align_run(tsdf_volume *dst, tsdf_volume *src, const AlignScratch &sc, const float start[16], Queue queue)
{
    double M[12];
    for (int i = 0; i < 12; ++i) M[i] = (double)start[i];
    hipLaunchKernelGGL(tsdfk::track_init, dim3(1), dim3(64), 0, dst->stream, sc.state, track_initial(M));
    HIP_TRY(hipGetLastError());
    int rc = fuse_after_src(dst, src, dst->align_src_ready);
    if (rc == TSDF_OK) rc = queue();
    if (rc == TSDF_OK) rc = fuse_src_after(dst, src, dst->align_done);
    if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(dst->h_align.get(), sc.state, sizeof(tsdfk::TrackState), hipMemcpyDeviceToHost, dst->stream));
    HIP_TRY(hipStreamSynchronize(dst->stream));
    return TSDF_OK;
}

int align_lattice_ok(const char *who, const tsdf_volume *dst)
{
    const tsdf_config &c = dst->cfg;
    const int64_t lanes = (int64_t)((c.dim_x + tsdfk::kAlignTileX - 1) / tsdfk::kAlignTileX) *
                          ((c.dim_y + tsdfk::kAlignTileY - 1) / tsdfk::kAlignTileY) * c.dim_z * 64;
    if (lanes >= ((int64_t)1 << 31))
        return fail(TSDF_ERR_INVALID, "%s: dst has too many voxels for one pass (%lld lanes)", who, (long long)lanes);
    return TSDF_OK;
}

}  // namespace

extern "C" {

int tsdf_align_params_default(const tsdf_config *dst_cfg, tsdf_align_params *out)
{
    if (!dst_cfg || !out) return fail(TSDF_ERR_INVALID, "tsdf_align_params_default: NULL argument");
    // choices, not measurements
    out->weight_thresh = 0.9f;
    out->resid_thresh = 1.0f;            // one truncation distance between the two surfaces
    out->n_levels = 2;
    out->iters[0] = 10; out->iters[1] = 10; out->iters[2] = 0;
    out->min_pairs = 300;                // tsdf_track's figure
    out->eps_rot = 1e-5f;
    out->eps_trans = 1e-5f;
    return TSDF_OK;
}

int tsdf_align_volume(tsdf_volume *dst, tsdf_volume *src, const tsdf_align_params *p, const float guess_dst2src[16],
                      tsdf_align_result *out)
{
    const char *who = "tsdf_align_volume";
    int rc = align_checks(who, dst, src, p, "guess_dst2src", guess_dst2src, out);
    if (rc == TSDF_OK) rc = align_lattice_ok(who, dst);
    if (rc) return rc;
    AlignScratch sc;
    rc = align_scratch(dst, &sc);
    if (rc) return rc;
    float start[16];
    if (guess_dst2src) std::memcpy(start, guess_dst2src, sizeof start);
    else tsdf_host::multiply_matrix(src->base2world_inv, dst->cfg.base2world, start);
    rc = align_run(dst, src, sc, start, [&]() {
        int r = TSDF_OK;
        for (int l = p->n_levels - 1; l >= 0 && r == TSDF_OK; --l)
            for (int it = 0; it < p->iters[l] && r == TSDF_OK; ++it) r = align_iteration(dst, src, p, sc, l, false);
        return r;
    });
    if (rc) return rc;
    const tsdfk::TrackState &st = *dst->h_align.get();
    std::memset(out, 0, sizeof *out);
    for (int l = 0; l < 3; ++l) out->iters_run[l] = st.iters_run[l];
    out->pairs = st.inliers;
    out->rmse = st.inliers > 0 ? (float)std::sqrt(st.r2 / (double)st.inliers) : 0.0f;
    if (st.lost) {                         // the starting matrix's own bits, all 16
        out->status = 2;
        std::memcpy(out->dst2src, start, sizeof start);
    } else {
        int last = -1;                     // the finest level that ran
        for (int l = p->n_levels - 1; l >= 0; --l)
            if (p->iters[l] > 0) last = l;
        out->status = last >= 0 && st.done[last] ? 0 : 1;
        for (int k = 0; k < 12; ++k) out->dst2src[k] = (float)st.M[k];
        out->dst2src[15] = 1.0f;           // (the memset left 0 0 0 in front of it)
    }
    return TSDF_OK;
}

int tsdf_align_system(tsdf_volume *dst, tsdf_volume *src, const tsdf_align_params *p, const float dst2src[16], int32_t level,
                      double system_out[29])
{
    const char *who = "tsdf_align_system";
    if (!dst2src) return fail(TSDF_ERR_INVALID, "%s: NULL dst2src", who);
    if (p && p->n_levels >= 1 && p->n_levels <= 3 && (level < 0 || level >= p->n_levels))
        return fail(TSDF_ERR_INVALID, "%s: level %d is outside [0, n_levels = %d)", who, level, p->n_levels);
    int rc = align_checks(who, dst, src, p, "dst2src", dst2src, system_out);
    if (rc == TSDF_OK) rc = align_lattice_ok(who, dst);
    if (rc) return rc;
    AlignScratch sc;
    rc = align_scratch(dst, &sc);
    if (rc) return rc;
    rc = align_run(dst, src, sc, dst2src, [&]() { return align_iteration(dst, src, p, sc, level, true); });
    if (rc) return rc;
    std::memcpy(system_out, dst->h_align.get()->sys, sizeof(double) * tsdfk::kTrackTerms);
    return TSDF_OK;
}

}  // extern "C"
