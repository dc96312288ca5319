// tsdf_fuse_host.hip.h -- host side of merging and re-gridding (include/tsdf_hip.h: tsdf_fuse_*), included at the end of
// tsdf_capi.hip; tsdf_fuse.hip.h states the rule, tsdf_fuse_carry.hip.h that of the colours and labels carried along.
#pragma once

namespace {

int fuse_handle_ok(const char *who, const char *side, const tsdf_volume *v)
{
    const tsdf_config &c = v->cfg;
    if (v->group_owner) return fail(TSDF_ERR_INVALID, "%s: %s is a slab of a tsdf_group; merging needs whole-grid handles", who, side);
    if (c.z_begin != 0 || c.z_end != c.dim_z)
        return fail(TSDF_ERR_INVALID, "%s: %s is the z-slab [%d,%d) of %d slices; merging needs whole-grid handles", who, side,
                    c.z_begin, c.z_end, c.dim_z);
    return TSDF_OK;
}

// What every call that takes a destination and a source refuses about the two handles.
int fuse_pair_ok(const char *who, const tsdf_volume *dst, const tsdf_volume *src)
{
    if (dst == src) return fail(TSDF_ERR_INVALID, "%s: dst and src are the same handle", who);
    int rc = fuse_handle_ok(who, "dst", dst);
    if (rc == TSDF_OK) rc = fuse_handle_ok(who, "src", src);
    if (rc) return rc;
    if (dst->cfg.device != src->cfg.device)
        return fail(TSDF_ERR_INVALID, "%s: dst is on device %d, src on device %d", who, dst->cfg.device, src->cfg.device);
    return TSDF_OK;
}

// What is queued next on dst's stream runs after everything queued on src's stream so far.
int fuse_after_src(tsdf_volume *dst, tsdf_volume *src, hipEvent_t src_ready)
{
    if (src->stream == dst->stream) return TSDF_OK;
    HIP_TRY(hipEventRecord(src_ready, src->stream));
    HIP_TRY(hipStreamWaitEvent(dst->stream, src_ready, 0));
    return TSDF_OK;
}

// A later write to src must not overtake the reads queued on dst's stream so far.
int fuse_src_after(tsdf_volume *dst, tsdf_volume *src, hipEvent_t done)
{
    if (src->stream == dst->stream) return TSDF_OK;
    HIP_TRY(hipEventRecord(done, dst->stream));
    HIP_TRY(hipStreamWaitEvent(src->stream, done, 0));
    return TSDF_OK;
}

constexpr int kFuseWords = 8;   // the merge's four counts, then the four of the labels carried

// The body of tsdf_fuse_volume, tsdf_fuse_volume_at and tsdf_fuse_volume_carry: the merge with the first three rows of M as the
// pose.  carry (TSDF_FUSE_CARRY_*; the caller has checked that both handles hold what it names): the attributes' kernel is
// queued ahead of the merge's, so it reads the weights the merge is about to replace.
int fuse_volume_with(const char *who, tsdf_volume *dst, tsdf_volume *src, const tsdf_fuse_params *p, const float M[16],
                     tsdf_fuse_counts *counts, uint32_t carry = 0, tsdf_fuse_carry_counts *carry_counts = nullptr)
{
    if (!std::isfinite(p->weight_thresh)) return fail(TSDF_ERR_INVALID, "%s: weight_thresh is not finite", who);
    if (!std::isfinite(p->agree_tol) || !(p->agree_tol > 0.0f))
        return fail(TSDF_ERR_INVALID, "%s: agree_tol must be finite and > 0 (%g)", who, (double)p->agree_tol);
    if (p->write != 0 && p->write != 1) return fail(TSDF_ERR_INVALID, "%s: write must be 0 or 1 (%d)", who, p->write);
    int rc = bind_device(dst);           // the collected frames of both, through their batches where they have one
    if (rc == TSDF_OK) rc = bind_device(src);
    if (rc) return rc;
    if (!dst->d_fuse) {                  // all four or none
        DevPtr<unsigned long long> d;
        HostPtr<unsigned long long> h;
        Event ready, done;
        HIP_TRY(dev_alloc(d, kFuseWords * sizeof(unsigned long long)));
        HIP_TRY(host_alloc(h, kFuseWords * sizeof(unsigned long long), hipHostMallocDefault));
        HIP_TRY(event_create(ready));
        HIP_TRY(event_create(done));
        dst->d_fuse = std::move(d); dst->h_fuse = std::move(h);
        dst->fuse_src_ready = std::move(ready); dst->fuse_done = std::move(done);
    }
    const tsdf_config &cd = dst->cfg, &cs = src->cfg;
    tsdfk::FuseParams k;
    k.dt = dst->d_tsdf; k.dw = dst->d_weight;
    k.st = src->d_tsdf; k.sw = src->d_weight;
    for (int i = 0; i < 12; ++i) k.m[i] = M[i];
    const int sd[3] = {cs.dim_x, cs.dim_y, cs.dim_z}, dd[3] = {cd.dim_x, cd.dim_y, cd.dim_z};
    for (int i = 0; i < 3; ++i) {
        k.od[i] = cd.origin[i]; k.os[i] = cs.origin[i];
        k.hi[i] = (float)(sd[i] - 1);
        k.sdim[i] = sd[i]; k.ddim[i] = dd[i];
    }
    k.vsd = cd.voxel_size; k.vss = cs.voxel_size;
    k.ratio = cs.trunc_margin / cd.trunc_margin;
    k.wthr = p->weight_thresh; k.tol = p->agree_tol;
    k.write = p->write;
    k.counts = dst->d_fuse;
    HIP_TRY(hipMemsetAsync(dst->d_fuse, 0, kFuseWords * sizeof(unsigned long long), dst->stream));
    rc = fuse_after_src(dst, src, dst->fuse_src_ready);
    if (rc) return rc;
    const int quads = (cd.dim_x + 3) / 4;
    const dim3 grid((quads + 7) / 8, (cd.dim_y + 7) / 8, (cd.dim_z + 4 * tsdfk::kFuseZRun - 1) / (4 * tsdfk::kFuseZRun));
    const bool colour = (carry & TSDF_FUSE_CARRY_COLOUR) && p->write;   // colour has no counts: a dry run has nothing to do
    const bool labels = (carry & TSDF_FUSE_CARRY_LABELS) != 0;
    if (colour || labels) {              // (handles with either attribute have dim_x % 4 == 0: tsdf_*_enable)
        tsdfk::FuseCarryParams c;
        c.g = k;
        c.dcol = dst->d_colour; c.scol = src->d_colour;
        c.dlab = dst->d_label; c.dfp = dst->d_fp; c.dbp = dst->d_bp;
        c.slab = src->d_label; c.sfp = src->d_fp; c.sbp = src->d_bp;
        c.prob_thd = dst->prob_thd;
        c.counts = dst->d_fuse + 4;
        if (colour && labels)
            hipLaunchKernelGGL((tsdfk::fuse_carry<true, true>), grid, dim3(256), 0, dst->stream, c);
        else if (colour)
            hipLaunchKernelGGL((tsdfk::fuse_carry<true, false>), grid, dim3(256), 0, dst->stream, c);
        else
            hipLaunchKernelGGL((tsdfk::fuse_carry<false, true>), grid, dim3(256), 0, dst->stream, c);
        HIP_TRY(hipGetLastError());
    }
    if (cd.dim_x % 4 == 0)
        hipLaunchKernelGGL(tsdfk::fuse_volume<true>, grid, dim3(256), 0, dst->stream, k);
    else
        hipLaunchKernelGGL(tsdfk::fuse_volume<false>, grid, dim3(256), 0, dst->stream, k);
    HIP_TRY(hipGetLastError());
    rc = fuse_src_after(dst, src, dst->fuse_done);
    if (rc) return rc;
    if (p->write) {                      // later fused / classified Integrate launches must not trust stale summary words
        rc = rebuild_summary(dst);
        if (rc) return rc;
    }
    HIP_TRY(hipMemcpyAsync(dst->h_fuse.get(), dst->d_fuse, kFuseWords * sizeof(unsigned long long), hipMemcpyDeviceToHost, dst->stream));
    HIP_TRY(hipStreamSynchronize(dst->stream));
    if (counts) {
        counts->sampled = dst->h_fuse.get()[0];
        counts->both = dst->h_fuse.get()[1];
        counts->both_band = dst->h_fuse.get()[2];
        counts->agree_band = dst->h_fuse.get()[3];
    }
    if (carry_counts) {
        carry_counts->label_adopted = dst->h_fuse.get()[4];
        carry_counts->label_agreed = dst->h_fuse.get()[5];
        carry_counts->label_opposed = dst->h_fuse.get()[6];
        carry_counts->label_flipped = dst->h_fuse.get()[7];
    }
    return TSDF_OK;
}

}  // namespace

extern "C" {

int tsdf_fuse_params_default(const tsdf_config *dst_cfg, tsdf_fuse_params *out)
{
    if (!dst_cfg || !out) return fail(TSDF_ERR_INVALID, "tsdf_fuse_params_default: NULL argument");
    out->weight_thresh = 0.9f;
    out->agree_tol = 0.4f;   // two voxels of the default band of five: a choice
    out->write = 1;
    return TSDF_OK;
}

int tsdf_fuse_pose_default(const tsdf_config *dst_cfg, const tsdf_config *src_cfg, float dst2src[16])
{
    if (!dst_cfg || !src_cfg || !dst2src) return fail(TSDF_ERR_INVALID, "tsdf_fuse_pose_default: NULL argument");
    float inv[16] = {};                  // a singular base2world_src: the all-zero inverse, as tsdf_create keeps it
    tsdf_host::invert_matrix(src_cfg->base2world, inv);
    tsdf_host::multiply_matrix(inv, dst_cfg->base2world, dst2src);
    return TSDF_OK;
}

int tsdf_fuse_volume(tsdf_volume *dst, tsdf_volume *src, const tsdf_fuse_params *p, tsdf_fuse_counts *counts)
{
    const char *who = "tsdf_fuse_volume";
    if (!dst || !src || !p) return fail(TSDF_ERR_INVALID, "%s: NULL argument", who);
    const int rc = fuse_pair_ok(who, dst, src);
    if (rc) return rc;
    float M[16];
    tsdf_host::multiply_matrix(src->base2world_inv, dst->cfg.base2world, M);
    return fuse_volume_with(who, dst, src, p, M, counts);
}

int tsdf_fuse_volume_at(tsdf_volume *dst, tsdf_volume *src, const tsdf_fuse_params *p, const float dst2src[16],
                        tsdf_fuse_counts *counts)
{
    const char *who = "tsdf_fuse_volume_at";
    if (!dst || !src || !p) return fail(TSDF_ERR_INVALID, "%s: NULL argument", who);
    if (!dst2src) return fail(TSDF_ERR_INVALID, "%s: NULL dst2src", who);
    const int rc = fuse_pair_ok(who, dst, src);
    if (rc) return rc;
    for (int i = 0; i < 12; ++i)
        if (!std::isfinite(dst2src[i])) return fail(TSDF_ERR_INVALID, "%s: dst2src[%d] is not finite", who, i);
    return fuse_volume_with(who, dst, src, p, dst2src, counts);
}

int tsdf_fuse_volume_carry(tsdf_volume *dst, tsdf_volume *src, const tsdf_fuse_params *p, const float dst2src[16],
                           uint32_t carry, tsdf_fuse_counts *counts, tsdf_fuse_carry_counts *carry_counts)
{
    const char *who = "tsdf_fuse_volume_carry";
    if (!dst || !src || !p) return fail(TSDF_ERR_INVALID, "%s: NULL argument", who);
    const int rc = fuse_pair_ok(who, dst, src);
    if (rc) return rc;
    if (carry & ~(TSDF_FUSE_CARRY_COLOUR | TSDF_FUSE_CARRY_LABELS))
        return fail(TSDF_ERR_INVALID, "%s: carry has bits outside TSDF_FUSE_CARRY_COLOUR | TSDF_FUSE_CARRY_LABELS (%u)", who, carry);
    if (carry & TSDF_FUSE_CARRY_COLOUR) {
        if (!dst->d_colour) return fail(TSDF_ERR_INVALID, "%s: colour is not enabled on dst (tsdf_colour_enable)", who);
        if (!src->d_colour) return fail(TSDF_ERR_INVALID, "%s: colour is not enabled on src (tsdf_colour_enable)", who);
    }
    if (carry & TSDF_FUSE_CARRY_LABELS) {
        if (!dst->d_label) return fail(TSDF_ERR_INVALID, "%s: labels are not enabled on dst (tsdf_labels_enable)", who);
        if (!src->d_label) return fail(TSDF_ERR_INVALID, "%s: labels are not enabled on src (tsdf_labels_enable)", who);
    }
    float M[16];
    if (dst2src) {
        for (int i = 0; i < 12; ++i)
            if (!std::isfinite(dst2src[i])) return fail(TSDF_ERR_INVALID, "%s: dst2src[%d] is not finite", who, i);
    } else {
        tsdf_host::multiply_matrix(src->base2world_inv, dst->cfg.base2world, M);
    }
    return fuse_volume_with(who, dst, src, p, dst2src ? dst2src : M, counts, carry, carry_counts);
}

}  // extern "C"
