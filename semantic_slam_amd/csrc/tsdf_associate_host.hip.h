// tsdf_associate_host.hip.h -- host side of association (tsdf_associate_*, tsdf_batch_associate; tsdf_associate.hip.h states the counting
// rule, include/tsdf_hip.h the assignment), included at the end of tsdf_capi.hip after tsdf_raycast_host.hip.h, whose batch render it uses.
#pragma once

namespace {

constexpr int kAssocMaxMembers = 65536;   // keeps the member tiles within the launch's y limit (MT >= 9 at K = 256)

int assoc_params_ok(const char *who, const tsdf_associate_params *p)
{
    if (!p) return fail(TSDF_ERR_INVALID, "%s: NULL parameters", who);
    int rc = ray_params_ok(who, &p->ray);
    if (rc) return rc;
    if (!(std::isfinite(p->depth_tol_m) && p->depth_tol_m > 0.0f))
        return fail(TSDF_ERR_INVALID, "%s: depth_tol_m must be finite and > 0 (%g)", who, (double)p->depth_tol_m);
    if (p->min_pixels < 1) return fail(TSDF_ERR_INVALID, "%s: min_pixels %d is below 1", who, p->min_pixels);
    if (!(p->min_iou >= 0.0f && p->min_iou <= 1.0f))
        return fail(TSDF_ERR_INVALID, "%s: min_iou must lie in [0, 1] (%g)", who, (double)p->min_iou);
    if (p->one_to_one != 0 && p->one_to_one != 1)
        return fail(TSDF_ERR_INVALID, "%s: one_to_one must be 0 or 1 (%d)", who, p->one_to_one);
    return TSDF_OK;
}

int masks_ok(const char *who, int32_t k)     // (of segmentation too)
{
    if (k < 1 || k > tsdfk::kAssocMaxMasks)
        return fail(TSDF_ERR_INVALID, "%s: k = %d masks is outside 1..%d", who, k, tsdfk::kAssocMaxMasks);
    return TSDF_OK;
}

int assoc_sizes_ok(const char *who, int32_t k, int32_t n_members)
{
    int rc = masks_ok(who, k);
    if (rc) return rc;
    if (n_members < 1 || n_members > kAssocMaxMembers)
        return fail(TSDF_ERR_INVALID, "%s: n_members = %d is outside 1..%d", who, n_members, kAssocMaxMembers);
    return TSDF_OK;
}

int assoc_labels_ok(const char *who, const tsdf_associate_labels *l)
{
    if (l && (!l->mask_label || !l->mask_score || !l->member_label || !l->member_score))
        return fail(TSDF_ERR_INVALID, "%s: a label block needs all four arrays", who);
    return TSDF_OK;
}

size_t assoc_words(int K, int M) { return 3 * (size_t)K * M + 3 * (size_t)K + 4 * (size_t)M; }

// Zero the block and count, queued on s.
int launch_associate(hipStream_t s, const tsdf_associate_params *p, const int32_t *member, const float *rdepth, int M,
                            const float *depth, const uint8_t *masks, int K, uint32_t *counts)
{
    HIP_TRY(hipMemsetAsync(counts, 0, assoc_words(K, M) * sizeof(uint32_t), s));
    tsdfk::AssocParams k;
    k.member = member; k.rdepth = rdepth; k.depth = depth; k.masks = masks; k.counts = counts;
    k.n_px = (int64_t)p->ray.im_height * p->ray.im_width;
    k.n_quads = (k.n_px + 3) / 4;
    k.K = K; k.M = M; k.MT = tsdfk::assoc_tile_members(K, M);
    k.near_m = p->ray.near_m; k.far_m = p->ray.far_m; k.tol = p->depth_tol_m;
    const int tiles = (M + k.MT - 1) / k.MT;
    const int nb = (int)std::max<int64_t>(1, std::min<int64_t>((k.n_quads + 255) / 256, tsdfk::kAssocMaxBlocks));
    const size_t lds = (3 * (size_t)K * k.MT + 3 * (size_t)K + 4 * (size_t)k.MT) * sizeof(uint32_t);
    auto aligned = [](const void *q, uintptr_t a) { return (reinterpret_cast<uintptr_t>(q) & (a - 1)) == 0; };
    const bool vec = k.n_px % 4 == 0 && aligned(member, 16) && aligned(rdepth, 16) && aligned(depth, 16) && aligned(masks, 4);
    if (vec)
        hipLaunchKernelGGL(tsdfk::associate_count<true>, dim3(nb, tiles), dim3(256), lds, s, k);
    else
        hipLaunchKernelGGL(tsdfk::associate_count<false>, dim3(nb, tiles), dim3(256), lds, s, k);
    HIP_TRY(hipGetLastError());
    return TSDF_OK;
}

struct AssocCandidate {
    int k, m;
    uint64_t a, u;
};

// a1 / u1 > a2 / u2, exactly (u > 0; the products need up to 65 bits)
bool assoc_iou_greater(const AssocCandidate &x, const AssocCandidate &y)
{
    return (unsigned __int128)x.a * y.u > (unsigned __int128)y.a * x.u;
}

// The assignment of include/tsdf_hip.h on a count block (the arguments checked by the caller).
int assoc_assign(const char *who, const tsdf_associate_params *p, const uint32_t *counts, int K, int M,
                        const tsdf_associate_labels *labels, int32_t *assign_out, float *iou_out)
{
    const uint32_t *ov = counts, *mask = counts + 3 * (size_t)K * M, *mem = mask + 3 * (size_t)K;
    for (int k = 0; k < K; ++k)
        for (int m = 0; m < M; ++m) {
            const uint32_t a = ov[((size_t)k * M + m) * 3];
            if (a > mask[3 * k + 1] || a > mem[4 * m])
                return fail(TSDF_ERR_INVALID, "%s: inconsistent counts: overlap[%d][%d][agree] = %u exceeds mask[%d][1] = %u "
                            "or member[%d][0] = %u", who, k, m, a, k, mask[3 * k + 1], m, mem[4 * m]);
        }
    std::vector<AssocCandidate> cand;
    for (int k = 0; k < K; ++k)
        for (int m = 0; m < M; ++m) {
            const uint64_t a = ov[((size_t)k * M + m) * 3];
            const uint64_t u = (uint64_t)mask[3 * k + 1] + mem[4 * m] - a;     // >= a: the check above
            if (a < (uint64_t)p->min_pixels || !((double)a >= (double)p->min_iou * (double)u)) continue;
            if (labels && !(labels->mask_label[k] == labels->member_label[m] ||
                            labels->member_score[m] > 1.1f * labels->mask_score[k]))
                continue;
            cand.push_back({k, m, a, u});                                      // in (k, m) order
        }
    std::vector<const AssocCandidate *> pick(K, nullptr);
    if (p->one_to_one) {
        std::stable_sort(cand.begin(), cand.end(), assoc_iou_greater);        // equal IoUs keep (k, m) order
        std::vector<char> used_m(M, 0);
        for (const AssocCandidate &c : cand) {
            if (pick[c.k] || used_m[c.m]) continue;
            pick[c.k] = &c;
            used_m[c.m] = 1;
        }
    } else {
        for (const AssocCandidate &c : cand)
            if (!pick[c.k] || assoc_iou_greater(c, *pick[c.k])) pick[c.k] = &c;   // ties keep the lower m
    }
    for (int k = 0; k < K; ++k) {
        assign_out[k] = pick[k] ? pick[k]->m : -1;
        iou_out[k] = pick[k] ? (float)((double)pick[k]->a / (double)pick[k]->u) : 0.0f;
    }
    return TSDF_OK;
}

}  // namespace

extern "C" {

int tsdf_associate_params_default(const tsdf_config *cfg, tsdf_associate_params *out)
{
    if (!cfg || !out) return fail(TSDF_ERR_INVALID, "tsdf_associate_params_default: NULL argument");
    int rc = tsdf_raycast_params_default(cfg, &out->ray);
    if (rc) return rc;
    out->depth_tol_m = cfg->trunc_margin;
    out->min_pixels = 25;
    out->min_iou = 0.25f;
    out->one_to_one = 1;
    return TSDF_OK;
}

int tsdf_associate_count(int32_t device, const tsdf_associate_params *p, const int32_t *member_dev, const float *rdepth_dev,
                         int32_t n_members, const float *depth_dev, const uint8_t *masks_dev, int32_t k,
                         uint32_t *counts_host)
{
    const char *who = "tsdf_associate_count";
    if (!member_dev || !rdepth_dev || !depth_dev || !masks_dev || !counts_host)
        return fail(TSDF_ERR_INVALID, "%s: NULL argument", who);
    int rc = assoc_params_ok(who, p);
    if (rc == TSDF_OK) rc = assoc_sizes_ok(who, k, n_members);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(device));
    // the images may have been produced on a handle's (non-blocking) stream, which the null stream does not order against
    HIP_TRY(hipDeviceSynchronize());
    const size_t words = assoc_words(k, n_members);
    DevPtr<uint32_t> d_counts;
    HIP_TRY(dev_alloc(d_counts, words * sizeof(uint32_t)));
    rc = launch_associate(0, p, member_dev, rdepth_dev, n_members, depth_dev, masks_dev, k, d_counts);
    if (rc) return rc;
    HIP_TRY(hipMemcpy(counts_host, d_counts, words * sizeof(uint32_t), hipMemcpyDeviceToHost));
    return TSDF_OK;
}

int tsdf_associate_assign(const tsdf_associate_params *p, const uint32_t *counts_host, int32_t k, int32_t n_members,
                          const tsdf_associate_labels *labels, int32_t *assign_out, float *iou_out)
{
    const char *who = "tsdf_associate_assign";
    if (!counts_host || !assign_out || !iou_out) return fail(TSDF_ERR_INVALID, "%s: NULL argument", who);
    int rc = assoc_params_ok(who, p);
    if (rc == TSDF_OK) rc = assoc_sizes_ok(who, k, n_members);
    if (rc == TSDF_OK) rc = assoc_labels_ok(who, labels);
    if (rc) return rc;
    return assoc_assign(who, p, counts_host, k, n_members, labels, assign_out, iou_out);
}

int tsdf_batch_associate(tsdf_batch *b, const tsdf_associate_params *p, const float cam2world[16], const float *depth_dev,
                         const uint8_t *masks_dev, int32_t k, const tsdf_associate_labels *labels, uint32_t *counts_host,
                         int32_t *assign_out, float *iou_out)
{
    const char *who = "tsdf_batch_associate";
    if (!b || !cam2world || !depth_dev || !masks_dev || !assign_out || !iou_out)
        return fail(TSDF_ERR_INVALID, "%s: NULL argument", who);
    const int M = (int)b->vols.size();
    int rc = assoc_params_ok(who, p);
    if (rc == TSDF_OK) rc = assoc_sizes_ok(who, k, M);
    if (rc == TSDF_OK) rc = assoc_labels_ok(who, labels);
    if (rc) return rc;
    const tsdf_config &c0 = b->vols[0]->cfg;
    if (p->ray.im_height != c0.im_height || p->ray.im_width != c0.im_width)
        return fail(TSDF_ERR_INVALID, "%s: the render is %dx%d, the batch's frames %dx%d", who, p->ray.im_width,
                    p->ray.im_height, c0.im_width, c0.im_height);
    rc = batch_render_checks(who, b, &p->ray);   // then the collected frames
    if (rc) return rc;
    // scratch: member | render depth | counts (kept on the batch, grown with the image and the block)
    const size_t px = (size_t)p->ray.im_height * p->ray.im_width, words = assoc_words(k, M);
    tsdf_host::Regions r;
    const size_t o_m = r.add(px * 4), o_d = r.add(px * 4), o_c = r.add(words * sizeof(uint32_t));
    HIP_TRY(b->d_assoc.ensure(r.total()));
    HIP_TRY(b->h_assoc.ensure(words));
    char *base = b->d_assoc;
    int32_t *member = reinterpret_cast<int32_t *>(base + o_m);
    float *rdepth = reinterpret_cast<float *>(base + o_d);
    uint32_t *counts = reinterpret_cast<uint32_t *>(base + o_c);
    rc = batch_render(b, &p->ray, cam2world, rdepth, nullptr, member);
    if (rc == TSDF_OK) rc = launch_associate(b->stream, p, member, rdepth, M, depth_dev, masks_dev, k, counts);
    if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(b->h_assoc.get(), counts, words * sizeof(uint32_t), hipMemcpyDeviceToHost, b->stream));
    HIP_TRY(hipStreamSynchronize(b->stream));
    if (counts_host) std::memcpy(counts_host, b->h_assoc.get(), words * sizeof(uint32_t));
    return assoc_assign(who, p, b->h_assoc.get(), k, M, labels, assign_out, iou_out);
}

}  // extern "C"
