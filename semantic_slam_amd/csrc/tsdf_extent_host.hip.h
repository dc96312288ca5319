// tsdf_extent_host.hip.h -- host side of the extent calls (include/tsdf_hip.h: tsdf_extent_*, tsdf_volume_extent,
// tsdf_batch_extents; tsdf_group_extent is with the group, tsdf_group.hip.h), included at the end of tsdf_capi.hip;
// tsdf_extent.hip.h states the rule.
#pragma once

namespace {

// a record in HBM and in pinned memory is kExtentWords 64-bit words laid out as tsdf_extent
static_assert(sizeof(tsdf_extent) == tsdfk::kExtentWords * sizeof(unsigned long long), "tsdf_extent is 20 words");
static_assert(offsetof(tsdf_extent, border) == 11 * 8 && offsetof(tsdf_extent, lo) == tsdfk::kExtentSums * 8 &&
              offsetof(tsdf_extent, hi) == tsdfk::kExtentSums * 8 + 12, "tsdf_extent's layout is the kernels'");

int extent_params_ok(const char *who, const tsdf_extent_params *p)
{
    if (!std::isfinite(p->weight_thresh)) return fail(TSDF_ERR_INVALID, "%s: weight_thresh is not finite", who);
    if (!std::isfinite(p->band) || !(p->band > 0.0f) || !(p->band <= 1.0f))
        return fail(TSDF_ERR_INVALID, "%s: band must be finite and in (0, 1] (%g)", who, (double)p->band);
    if (p->margin < 0) return fail(TSDF_ERR_INVALID, "%s: margin must be >= 0 (%d)", who, p->margin);
    return TSDF_OK;
}

// The second moments are sums of at most `voxels` products of two indices below the largest global dim.
int extent_volume_ok(const char *who, const tsdf_volume *v)
{
    const tsdf_config &c = v->cfg;
    const unsigned __int128 m = (unsigned __int128)std::max(c.dim_x, std::max(c.dim_y, c.dim_z));
    if ((unsigned __int128)v->geo.n_vox * m * m >> 64)
        return fail(TSDF_ERR_INVALID, "%s: %lld voxels of a %dx%dx%d grid: the second moments could reach 2^64", who,
                    (long long)v->geo.n_vox, c.dim_x, c.dim_y, c.dim_z);
    return TSDF_OK;
}

// The kernels' view of a handle; its partial records are filled in by the caller.
tsdfk::ExtentVolume extent_volume(const tsdf_volume *v)
{
    const tsdf_config &c = v->cfg;
    tsdfk::ExtentVolume e = {};
    e.t = v->d_tsdf; e.w = v->d_weight;
    e.dim[0] = c.dim_x; e.dim[1] = c.dim_y; e.dim[2] = c.dim_z;
    e.z_begin = c.z_begin;
    e.tiles_x = ((c.dim_x + 3) / 4 + 7) / 8;
    e.tiles = e.tiles_x * ((c.dim_y + 7) / 8);       // <= dim_x * dim_y / 256 + ...: tsdf_create bounds a slice by 2^31
    return e;
}

// workgroups per slice: four wavefronts of kExtentTilesPerWave tiles each
int extent_blocks(const tsdfk::ExtentVolume &e)
{
    return std::max(1, (e.tiles + 4 * tsdfk::kExtentTilesPerWave - 1) / (4 * tsdfk::kExtentTilesPerWave));
}

tsdfk::ExtentRule extent_rule(const tsdf_extent_params *p)
{
    tsdfk::ExtentRule r;
    r.wthr = p->weight_thresh; r.band = p->band; r.margin = p->margin;
    return r;
}

}  // namespace

extern "C" {

int tsdf_extent_params_default(const tsdf_config *cfg, tsdf_extent_params *out)
{
    if (!cfg || !out) return fail(TSDF_ERR_INVALID, "tsdf_extent_params_default: NULL argument");
    out->weight_thresh = 0.9f;
    out->band = 1.0f;
    out->margin = (int32_t)ceilf(cfg->trunc_margin / cfg->voxel_size);   // the band in voxels: 5 for the reference's grid
    return TSDF_OK;
}

int tsdf_volume_extent(tsdf_volume *v, const tsdf_extent_params *p, tsdf_extent *out)
{
    const char *who = "tsdf_volume_extent";
    if (!v || !p || !out) return fail(TSDF_ERR_INVALID, "%s: NULL argument", who);
    int rc = extent_params_ok(who, p);
    if (rc == TSDF_OK) rc = extent_volume_ok(who, v);
    if (rc) return rc;
    rc = bind_device(v);                 // the collected frames, through its batch or group where it has one
    if (rc) return rc;
    const int nz = v->cfg.z_end - v->cfg.z_begin;
    tsdfk::ExtentVolume e = extent_volume(v);
    const int blocks = extent_blocks(e);
    e.first_partial = 0;
    e.n_partials = blocks * nz;
    if (!v->d_extent) {                  // both or neither
        DevPtr<unsigned long long> d;
        HostPtr<unsigned long long> h;
        HIP_TRY(dev_alloc(d, (size_t)(1 + e.n_partials) * sizeof(tsdf_extent)));
        HIP_TRY(host_alloc(h, sizeof(tsdf_extent), hipHostMallocDefault));
        v->d_extent = std::move(d); v->h_extent = std::move(h);
    }
    unsigned long long *record = v->d_extent, *partials = record + tsdfk::kExtentWords;
    const tsdfk::ExtentRule rule = extent_rule(p);
    if (nz > 0) {                        // (tsdf_create bounds a slab's slices by the launch limit)
        const dim3 grid((unsigned)blocks, 1, (unsigned)nz);
        if (v->cfg.dim_x % 4 == 0)
            hipLaunchKernelGGL((tsdfk::extent_partials<true, false>), grid, dim3(256), 0, v->stream, e, nullptr, nullptr, rule, partials);
        else
            hipLaunchKernelGGL((tsdfk::extent_partials<false, false>), grid, dim3(256), 0, v->stream, e, nullptr, nullptr, rule, partials);
    }
    hipLaunchKernelGGL(tsdfk::extent_finish<false>, dim3(1), dim3(tsdfk::kExtentFinishGroups * tsdfk::kExtentWords), 0, v->stream,
                       e, nullptr, partials, record);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(v->h_extent.get(), record, sizeof(tsdf_extent), hipMemcpyDeviceToHost, v->stream));
    HIP_TRY(hipStreamSynchronize(v->stream));
    std::memcpy(out, v->h_extent.get(), sizeof(tsdf_extent));
    return TSDF_OK;
}

int tsdf_batch_extents(tsdf_batch *b, const tsdf_extent_params *p, tsdf_extent *out)
{
    const char *who = "tsdf_batch_extents";
    if (!b || !p || !out) return fail(TSDF_ERR_INVALID, "%s: NULL argument", who);
    int rc = extent_params_ok(who, p);
    for (size_t i = 0; i < b->vols.size() && rc == TSDF_OK; ++i) rc = extent_volume_ok(who, b->vols[i]);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(b->device));
    for (tsdf_volume *v : b->vols) {     // the batch's collected frames, then any a member collected through its own handle
        rc = bind_device(v);
        if (rc) return rc;
    }
    const int M = (int)b->vols.size();
    if (!b->d_extent) {                  // all or none
        Staged<tsdfk::ExtentVolume> vols;
        HIP_TRY(host_alloc(vols.host, (size_t)M * sizeof(tsdfk::ExtentVolume), hipHostMallocDefault));
        HIP_TRY(dev_alloc(vols.dev, (size_t)M * sizeof(tsdfk::ExtentVolume)));
        int blocks = 1;
        for (int i = 0; i < M; ++i) {
            vols.host[i] = extent_volume(b->vols[i]);
            blocks = std::max(blocks, extent_blocks(vols.host[i]));
        }
        int first_slice = 0;             // the slice map lists the members in order, every slice of each (tsdf_batch_create)
        for (int i = 0; i < M; ++i) {
            const int nz = b->vols[i]->cfg.z_end - b->vols[i]->cfg.z_begin;
            vols.host[i].first_partial = first_slice * blocks;
            vols.host[i].n_partials = nz * blocks;
            first_slice += nz;
        }
        DevPtr<unsigned long long> d;
        HostPtr<unsigned long long> h;
        HIP_TRY(dev_alloc(d, ((size_t)M + (size_t)b->total_slices * blocks) * sizeof(tsdf_extent)));
        HIP_TRY(host_alloc(h, (size_t)M * sizeof(tsdf_extent), hipHostMallocDefault));
        HIP_TRY(hipMemcpy(vols.dev, vols.host, (size_t)M * sizeof(tsdfk::ExtentVolume), hipMemcpyHostToDevice));
        b->d_extent = std::move(d); b->h_extent = std::move(h);
        b->extent_vols = std::move(vols);
        b->extent_blocks = blocks;
    }
    unsigned long long *records = b->d_extent, *partials = records + (size_t)M * tsdfk::kExtentWords;
    const tsdfk::ExtentVolume none = {};
    if (b->total_slices > 0)             // every member's dim_x is a multiple of 4 (tsdf_batch_create)
        hipLaunchKernelGGL((tsdfk::extent_partials<true, true>), dim3((unsigned)b->extent_blocks, 1, (unsigned)b->total_slices), dim3(256), 0,
                           b->stream, none, b->extent_vols.dev.get(), b->d_slice_map.get(), extent_rule(p), partials);
    hipLaunchKernelGGL(tsdfk::extent_finish<true>, dim3((unsigned)M), dim3(tsdfk::kExtentFinishGroups * tsdfk::kExtentWords), 0, b->stream,
                       none, b->extent_vols.dev.get(), partials, records);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(b->h_extent.get(), records, (size_t)M * sizeof(tsdf_extent), hipMemcpyDeviceToHost, b->stream));
    HIP_TRY(hipStreamSynchronize(b->stream));
    std::memcpy(out, b->h_extent.get(), (size_t)M * sizeof(tsdf_extent));
    return TSDF_OK;
}

int tsdf_extent_combine(const tsdf_extent *a, const tsdf_extent *b, tsdf_extent *out)
{
    if (!a || !b || !out) return fail(TSDF_ERR_INVALID, "tsdf_extent_combine: NULL argument");
    tsdf_extent r = *a;
    r.n_observed += b->n_observed;
    r.n_surface += b->n_surface;
    for (int i = 0; i < 3; ++i) r.sum[i] += b->sum[i];
    for (int i = 0; i < 6; ++i) { r.sum2[i] += b->sum2[i]; r.border[i] += b->border[i]; }
    for (int i = 0; i < 3; ++i) { r.lo[i] = std::min(r.lo[i], b->lo[i]); r.hi[i] = std::max(r.hi[i], b->hi[i]); }
    *out = r;
    return TSDF_OK;
}

int tsdf_extent_metric(const tsdf_config *cfg, const tsdf_extent *e, struct tsdf_extent_metric *out)
{
    const char *who = "tsdf_extent_metric";
    if (!cfg || !e || !out) return fail(TSDF_ERR_INVALID, "%s: NULL argument", who);
    if (e->n_surface == 0) return fail(TSDF_ERR_INVALID, "%s: the record has no surface voxel (n_surface == 0)", who);
    const double n = (double)e->n_surface, vs = (double)cfg->voxel_size;
    double mean[3];
    for (int i = 0; i < 3; ++i) {
        mean[i] = (double)e->sum[i] / n;
        out->centroid_base[i] = (double)cfg->origin[i] + mean[i] * vs;
        out->lo_base[i] = (double)cfg->origin[i] + ((double)e->lo[i] - 0.5) * vs;
        out->hi_base[i] = (double)cfg->origin[i] + ((double)e->hi[i] + 0.5) * vs;
    }
    const float *B = cfg->base2world;
    for (int i = 0; i < 3; ++i)
        out->centroid_world[i] = (((double)B[4 * i] * out->centroid_base[0] + (double)B[4 * i + 1] * out->centroid_base[1]) +
                                  (double)B[4 * i + 2] * out->centroid_base[2]) + (double)B[4 * i + 3];
    const int ia[6] = {0, 1, 2, 0, 0, 1}, ib[6] = {0, 1, 2, 1, 2, 2};   // xx, yy, zz, xy, xz, yz
    for (int k = 0; k < 6; ++k) out->cov_base[k] = ((double)e->sum2[k] / n - mean[ia[k]] * mean[ib[k]]) * (vs * vs);
    return TSDF_OK;
}

int tsdf_extent_regrid(const tsdf_config *cfg, const tsdf_extent *e, int32_t pad_voxels, int32_t dim_multiple, tsdf_config *out_cfg)
{
    const char *who = "tsdf_extent_regrid";
    if (!cfg || !e || !out_cfg) return fail(TSDF_ERR_INVALID, "%s: NULL argument", who);
    if (e->n_surface == 0) return fail(TSDF_ERR_INVALID, "%s: the record has no surface voxel (n_surface == 0)", who);
    if (pad_voxels < 0) return fail(TSDF_ERR_INVALID, "%s: pad_voxels must be >= 0 (%d)", who, pad_voxels);
    if (dim_multiple < 1) return fail(TSDF_ERR_INVALID, "%s: dim_multiple must be >= 1 (%d)", who, dim_multiple);
    tsdf_config c = *cfg;
    int32_t *dim[3] = {&c.dim_x, &c.dim_y, &c.dim_z};
    for (int i = 0; i < 3; ++i) {
        if (e->hi[i] < e->lo[i]) return fail(TSDF_ERR_INVALID, "%s: the record's bounds are empty on axis %d (lo %d, hi %d)", who, i, e->lo[i], e->hi[i]);
        const int64_t first = (int64_t)e->lo[i] - pad_voxels;
        int64_t d = (int64_t)e->hi[i] - e->lo[i] + 1 + 2 * (int64_t)pad_voxels;
        d = (d + dim_multiple - 1) / dim_multiple * dim_multiple;
        if (d > 0x7fffffff || first < -0x7fffffff)
            return fail(TSDF_ERR_INVALID, "%s: axis %d of the proposed grid does not fit 32 bits (%lld voxels from index %lld)", who, i,
                        (long long)d, (long long)first);
        const float steps = (float)(int32_t)first;              // two rounded float32 operations: the product, the sum
        const float shift = steps * cfg->voxel_size;
        c.origin[i] = cfg->origin[i] + shift;
        *dim[i] = (int32_t)d;
    }
    c.z_begin = 0;
    c.z_end = c.dim_z;
    if (config_ok(&c) != TSDF_OK) {      // what tsdf_create would say
        const std::string why = g_last_error;
        return fail(TSDF_ERR_INVALID, "%s: the proposed %dx%dx%d grid would be refused: %s", who, c.dim_x, c.dim_y, c.dim_z, why.c_str());
    }
    *out_cfg = c;
    return TSDF_OK;
}

}  // extern "C"
