// tsdf_batch_host.hip.h -- host side of batched per-object volumes (include/tsdf_hip.h: tsdf_batch_create .. tsdf_batch_integrate_device),
// included at the end of tsdf_capi.hip, which declares struct tsdf_batch and, ahead of bind_device, batch_flush and batch_collect.
// The batch's raycast, association, joint tracking and extents are with their features.
#pragma once

namespace {

// Apply the frames the batch has collected: one fused launch per member, in member order, on the batch's stream.
int batch_flush(tsdf_batch *b)
{
    if (b->pend_count == 0 || b->in_flush) return TSDF_OK;
    b->in_flush = true;
    const int n = b->pend_count, members = (int)b->vols.size();
    b->pend_count = 0;
    const size_t px = (size_t)b->vols[0]->cfg.im_height * b->vols[0]->cfg.im_width;
    const float *ptrs[tsdfk::kMaxFramesPerLaunch];
    for (int f = 0; f < n; ++f) ptrs[f] = b->d_depth_pool + (size_t)f * px;
    int rc = TSDF_OK;
    if (hipSetDevice(b->device) != hipSuccess) rc = fail(TSDF_ERR_HIP, "tsdf_batch: hipSetDevice failed");
    // fork: the side streams start when everything queued on the batch's stream so far (the frames' copies) is done
    const int lanes = tsdf_host::batch_lanes(members);
    hipError_t e = hipSuccess;
    if (rc == TSDF_OK && lanes > 1) {
        if (!b->collected) {      // all or none
            Event collected, side_done[kBatchSideStreams];
            Stream side[kBatchSideStreams];
            e = event_create(collected);
            for (int k = 0; k < kBatchSideStreams && e == hipSuccess; ++k) {
                e = stream_create(side[k]);
                if (e == hipSuccess) e = event_create(side_done[k]);
            }
            if (e == hipSuccess) {
                b->collected = std::move(collected);
                for (int k = 0; k < kBatchSideStreams; ++k) { b->side[k] = std::move(side[k]); b->side_done[k] = std::move(side_done[k]); }
            }
        }
        if (e == hipSuccess) e = hipEventRecord(b->collected, b->stream);
        for (int k = 0; k < lanes && e == hipSuccess; ++k) e = hipStreamWaitEvent(b->side[k], b->collected, 0);
        if (e != hipSuccess) rc = fail(TSDF_ERR_HIP, "tsdf_batch: side streams: %s", hipGetErrorString(e));
    }
    for (int i = 0; i < members && rc == TSDF_OK; ++i) {
        tsdf_volume *v = b->vols[i];
        const uint8_t *const *masks = b->pend_mask.data() + (size_t)i * tsdfk::kMaxFramesPerLaunch;
        const float *c2b = b->pend_c2b.data() + (size_t)i * tsdfk::kMaxFramesPerLaunch * 16;
        if (lanes > 1) v->stream = b->side[i % lanes];
        rc = apply_collected(v, ptrs, masks, c2b, n);
        v->stream = b->stream;
    }
    // join: whatever follows on the batch's stream (the next frames' copies into the pool, a download) comes after them
    for (int k = 0; k < lanes && lanes > 1; ++k) {
        if (hipEventRecord(b->side_done[k], b->side[k]) != hipSuccess || hipStreamWaitEvent(b->stream, b->side_done[k], 0) != hipSuccess) {
            (void)hipDeviceSynchronize();   // never leave the streams unordered
            if (rc == TSDF_OK) rc = fail(TSDF_ERR_HIP, "tsdf_batch: joining the side streams failed");
        }
    }
    b->in_flush = false;
    return rc;
}

// Collect one frame for every member: the depth image once, the masks by one gather launch, the poses composed now.
// Everything is queued on the batch's stream, so the caller's buffers are free for reuse under that stream's order and the
// pool is not overwritten before the launches that read it have run.
int batch_collect(tsdf_batch *b, const float *depth_dev, const uint8_t *const *masks_dev, const float cam2world[16])
{
    const int members = (int)b->vols.size(), slot = b->pend_count;
    const size_t px = (size_t)b->vols[0]->cfg.im_height * b->vols[0]->cfg.im_width;
    if (!b->d_depth_pool) {
        HIP_TRY(dev_alloc(b->d_depth_pool, (size_t)tsdfk::kMaxFramesPerLaunch * px * sizeof(float)));
        b->pend_c2b.assign((size_t)members * tsdfk::kMaxFramesPerLaunch * 16, 0.0f);
        b->pend_mask.assign((size_t)members * tsdfk::kMaxFramesPerLaunch, nullptr);
    }
    bool any_mask = false;
    for (int i = 0; i < members && masks_dev; ++i) any_mask = any_mask || masks_dev[i] != nullptr;
    if (any_mask && !b->d_mask_pool)
        HIP_TRY(dev_alloc(b->d_mask_pool, (size_t)tsdfk::kMaxFramesPerLaunch * members * px));
    HIP_TRY(hipMemcpyAsync(b->d_depth_pool + (size_t)slot * px, depth_dev, px * sizeof(float), hipMemcpyDeviceToDevice, b->stream));
    for (int i0 = 0; i0 < members && any_mask; i0 += tsdfk::kGatherMasks) {
        tsdfk::MaskGatherParams gp;
        const int m = std::min(tsdfk::kGatherMasks, members - i0);
        bool some = false;
        for (int k = 0; k < tsdfk::kGatherMasks; ++k) {
            gp.src[k] = k < m ? masks_dev[i0 + k] : nullptr;
            gp.dst[k] = k < m ? b->d_mask_pool + ((size_t)slot * members + i0 + k) * px : nullptr;
            some = some || gp.src[k] != nullptr;
        }
        gp.bytes = px;
        if (some) hipLaunchKernelGGL(tsdfk::gather_masks, dim3((unsigned)((px + 4095) / 4096), (unsigned)m), dim3(256), 0, b->stream, gp);
    }
    HIP_TRY(hipGetLastError());
    for (int i = 0; i < members; ++i) {
        tsdf_volume *v = b->vols[i];
        float *c2b = b->pend_c2b.data() + ((size_t)i * tsdfk::kMaxFramesPerLaunch + slot) * 16;
        compose_cam2base(v, cam2world, c2b);   // each object has its own base frame (ref: src/Object.cpp:23-29)
        std::memcpy(v->last_cam2base, c2b, 16 * sizeof(float));
        b->pend_mask[(size_t)i * tsdfk::kMaxFramesPerLaunch + slot] =
            (masks_dev && masks_dev[i]) ? b->d_mask_pool + ((size_t)slot * members + i) * px : nullptr;
    }
    b->pend_count = slot + 1;
    if (b->pend_count >= std::min(b->vols[0]->defer_n, (int)tsdfk::kMaxFramesPerLaunch)) return batch_flush(b);
    return TSDF_OK;
}

}  // namespace

extern "C" {

int tsdf_batch_destroy(tsdf_batch *b)
{
    if (!b) return TSDF_OK;
    (void)hipSetDevice(b->device);
    if (b->stream) (void)hipStreamSynchronize(b->stream);
    for (tsdf_volume *v : b->vols) {
        if (v) { v->stream = v->own_stream; v->owner = nullptr; tsdf_destroy(v); }
    }
    for (Stream &side : b->side)
        if (side) (void)hipStreamSynchronize(side);
    delete b;            // the owners release the batch's memory, events and streams
    return TSDF_OK;
}

int tsdf_batch_create(const tsdf_config *cfgs, int32_t n, tsdf_batch **out)
{
    if (!cfgs || !out || n <= 0) return fail(TSDF_ERR_INVALID, "tsdf_batch_create: bad argument");
    *out = nullptr;
    for (int i = 0; i < n; ++i) {
        if (cfgs[i].device != cfgs[0].device || cfgs[i].im_height != cfgs[0].im_height ||
            cfgs[i].im_width != cfgs[0].im_width)
            return fail(TSDF_ERR_INVALID, "tsdf_batch_create: volume %d differs in device or image size", i);
        if (cfgs[i].dim_x % 4 != 0)
            return fail(TSDF_ERR_INVALID, "tsdf_batch_create: volume %d: dim_x must be a multiple of 4", i);
    }
    tsdf_batch *b = new (std::nothrow) tsdf_batch();
    if (!b) return fail(TSDF_ERR_INVALID, "tsdf_batch_create: out of host memory");
    b->device = cfgs[0].device;
    auto cleanup = [&](int code) { tsdf_batch_destroy(b); return code; };
    std::vector<int2> map;
    for (int i = 0; i < n; ++i) {
        tsdf_volume *v = nullptr;
        int rc = create_volume(&cfgs[i], true, &v);
        if (rc) return cleanup(rc);
        b->vols.push_back(v);
        const int nz = cfgs[i].z_end - cfgs[i].z_begin;
        for (int z = 0; z < nz; ++z) map.push_back(make_int2(i, z));
        b->max_blocks = std::max(b->max_blocks, (int)tsdf_host::grid_flat(v->geo).x);
    }
    b->total_slices = (int)map.size();
    if (b->total_slices > 65535) return cleanup(fail(TSDF_ERR_INVALID, "tsdf_batch_create: %d slices in total exceed the launch limit 65535", b->total_slices));
    hipError_t e = hipSetDevice(b->device);
    if (e == hipSuccess) e = stream_create(b->stream);
    if (e == hipSuccess && !map.empty()) e = dev_alloc(b->d_slice_map, map.size() * sizeof(int2));
    if (e == hipSuccess && !map.empty()) e = hipMemcpy(b->d_slice_map, map.data(), map.size() * sizeof(int2), hipMemcpyHostToDevice);
    for (auto &s : b->blocks.slots) {
        if (e == hipSuccess) e = host_alloc(s.params.host, n * sizeof(tsdfk::IntegrateParams), hipHostMallocDefault);
        if (e == hipSuccess) e = dev_alloc(s.params.dev, n * sizeof(tsdfk::IntegrateParams));
        if (e == hipSuccess) e = host_alloc(s.poses.host, n * sizeof(tsdfk::FramePose), hipHostMallocDefault);
        if (e == hipSuccess) e = dev_alloc(s.poses.dev, n * sizeof(tsdfk::FramePose));
        if (e == hipSuccess) e = event_create(s.done);
    }
    if (e != hipSuccess) return cleanup(fail(TSDF_ERR_HIP, "tsdf_batch_create: %s", hipGetErrorString(e)));
    for (tsdf_volume *v : b->vols) {   // creation fills ran on each volume's own stream: finish them, then share ours
        if (hipStreamSynchronize(v->stream) != hipSuccess) return cleanup(fail(TSDF_ERR_HIP, "tsdf_batch_create: sync failed"));
        v->stream = b->stream;
        v->owner = b;
    }
    *out = b;
    return TSDF_OK;
}

int tsdf_batch_size(const tsdf_batch *b) { return b ? (int)b->vols.size() : 0; }

int tsdf_batch_volume(tsdf_batch *b, int32_t i, tsdf_volume **vol)
{
    if (!b || !vol || i < 0 || i >= (int)b->vols.size()) return fail(TSDF_ERR_INVALID, "tsdf_batch_volume: bad argument");
    *vol = b->vols[i];
    return TSDF_OK;
}

int tsdf_batch_sync(tsdf_batch *b)
{
    if (!b) return fail(TSDF_ERR_INVALID, "tsdf_batch_sync: NULL handle");
    HIP_TRY(hipSetDevice(b->device));
    int rc = batch_flush(b);
    if (rc) return rc;
    HIP_TRY(hipStreamSynchronize(b->stream));
    return TSDF_OK;
}

int tsdf_batch_integrate_device(tsdf_batch *b, const float *depth_dev, const uint8_t *const *masks_dev,
                                const float cam2world[16])
{
    if (!b || !depth_dev || !cam2world) return fail(TSDF_ERR_INVALID, "tsdf_batch_integrate_device: NULL argument");
    HIP_TRY(hipSetDevice(b->device));
    if (b->total_slices == 0) return TSDF_OK;
    const int n = (int)b->vols.size();
    for (tsdf_volume *v : b->vols)
        if (v->pend_count > 0) { int rc = flush_pending(v); if (rc) return rc; }   // frames given to a borrowed handle come first
    // Deferral as for a single handle (tsdf_set_deferral on the FIRST member switches it), where it pays (tsdf_host::batch_defers)
    {
        bool defer = b->vols[0]->defer_n > 1;
        int64_t total = 0;
        for (tsdf_volume *v : b->vols) { defer = defer && can_fuse(v); total += v->geo.n_vox; }
        defer = defer && tsdf_host::batch_defers(n, total);
        if (defer) return batch_collect(b, depth_dev, masks_dev, cam2world);
        int rc = batch_flush(b);   // the policy changed between calls (tsdf_set_deferral, a kernel variant)
        if (rc) return rc;
    }
    for (tsdf_volume *v : b->vols) {   // the batched kernel maintains the summary, but not the weight runs (on the batch's stream, which the members share)
        int rc = summary_before(v, tsdf_host::Keeps::Bits);
        if (rc) return rc;
    }
    decltype(b->blocks)::Slot *s = nullptr;
    HIP_TRY(b->blocks.take(&s));
    tsdfk::IntegrateParams *const h_params = s->params.host, *const d_params = s->params.dev;
    tsdfk::FramePose *const h_poses = s->poses.host, *const d_poses = s->poses.dev;
    for (int i = 0; i < n; ++i) {
        tsdf_volume *v = b->vols[i];
        float c2b[16];
        compose_cam2base(v, cam2world, c2b);   // each object has its own base frame (ref: src/Object.cpp:23-29)
        std::memcpy(v->last_cam2base, c2b, sizeof c2b);
        const tsdfk::IntegrateParams q = make_params(v, depth_dev, masks_dev ? masks_dev[i] : nullptr, c2b, 4);
        h_params[i] = q;
        pose_from_params(h_poses[i], q);
    }
    // Instance masks given: every object sees only its own instance (ref: src/Engine.cpp:192-193), so most workgroups of
    // most objects see nothing.  Tile tables of depth x mask per object, the class of every workgroup of the launch
    // (one thread each), and the launch's untouched workgroups leave at once.  (First volume on variant 7: never.)
    bool any_mask = false;
    for (int i = 0; i < n && masks_dev; ++i) any_mask = any_mask || masks_dev[i] != nullptr;
    bool same_range = true;   // one tile table per object, but all made with one depth-range test
    for (int i = 1; i < n; ++i) same_range = same_range && b->vols[i]->cfg.max_depth == b->vols[0]->cfg.max_depth;
    int64_t launch_voxels = 0;
    for (tsdf_volume *v : b->vols) launch_voxels += v->geo.n_vox;
    // ... when the launch is large enough, and not for many small volumes (tsdf_host::batch_classifies)
    const bool classify = any_mask && same_range && tsdf_host::batch_classifies(variant_of(b->vols[0]->variant).classify, n, launch_voxels) &&
                          tiles_fit(h_params[0].tiles_w, h_params[0].tiles_h);
    if (classify) {
        // one coarse table per member, laid out as a launch's table slot lays out its frames' coarse ones
        const size_t per = tsdf_host::table_slot_layout(b->vols[0]->cfg, b->vols[0]->geo.tile, false).coarse_elems;
        if (!b->d_tiles) {      // (and, in the measurement build, the class table beside them: both or neither)
            DevPtr<float2> tiles;
            DevPtr<uint8_t> wg_class;
            HIP_TRY(dev_alloc(tiles, (size_t)n * per * sizeof(float2)));
            if (kExperiments) HIP_TRY(dev_alloc(wg_class, (size_t)b->max_blocks * b->total_slices));
            b->d_tiles = std::move(tiles); b->d_wg_class = std::move(wg_class);
            b->tiles_per_object = per;
        }
        std::vector<const float *> depths((size_t)n, depth_dev);
        int rc = build_tile_tables(b->stream, b->vols[0]->cfg, h_params[0], depths.data(), masks_dev, n, b->d_tiles);
        if (rc) return rc;
        for (int i = 0; i < n; ++i) h_poses[i].tiles = b->d_tiles + (size_t)i * per;
    }
    HIP_TRY(hipMemcpyAsync(d_params, h_params, n * sizeof(tsdfk::IntegrateParams), hipMemcpyHostToDevice, b->stream));
    HIP_TRY(hipMemcpyAsync(d_poses, h_poses, n * sizeof(tsdfk::FramePose), hipMemcpyHostToDevice, b->stream));
    dim3 block(64, 4, 1), grid(b->max_blocks, 1, b->total_slices);
    // a class per wavefront brick (every member has a brick view: dim_x % 4 == 0 is a condition of tsdf_batch_create)
    int brick_blocks = 0;
    bool bricks = classify && !(kExperiments && b->vols[0]->variant == 11);
    for (int i = 0; i < n && bricks; ++i) {
        bricks = b->vols[i]->geo.brick_q > 0;
        brick_blocks = std::max(brick_blocks, tsdf_host::brick_blocks(b->vols[i]->geo));
    }
    if (bricks) {
        // z index of the brick launches: slice groups (rebuilt when a member's brick depth changed: tsdf_set_brick_shape)
        bool same = b->d_group_map != nullptr && (int)b->group_s.size() == n;
        for (int i = 0; i < n && same; ++i) same = b->group_s[i] == h_params[i].brick_s;
        if (!same) {
            std::vector<int2> gmap;
            b->group_s.assign((size_t)n, 1);
            for (int i = 0; i < n; ++i) {
                b->group_s[i] = b->vols[i]->geo.brick_s;
                for (int g = 0; g < b->vols[i]->geo.nz_groups; ++g) gmap.push_back(make_int2(i, g));
            }
            HIP_TRY(hipStreamSynchronize(b->stream));
            HIP_TRY(dev_alloc(b->d_group_map, std::max<size_t>(gmap.size(), 1) * sizeof(int2)));
            HIP_TRY(hipMemcpy(b->d_group_map, gmap.data(), gmap.size() * sizeof(int2), hipMemcpyHostToDevice));
            b->total_groups = (int)gmap.size();
        }
        const tsdf_host::BrickGrid bg = tsdf_host::brick_grid(brick_blocks, b->total_groups);   // the widest member's blocks x all slice groups
        HIP_TRY(b->d_brick_class.ensure(bg.class_elems));
        hipLaunchKernelGGL(tsdfk::classify_bricks_batched, dim3((unsigned)((bg.class_elems + 255) / 256)), dim3(256), 0, b->stream,
                           d_params, d_poses, b->d_group_map, b->d_brick_class, brick_blocks, b->total_groups);
        hipLaunchKernelGGL((tsdfk::integrate_multi_batched_bricks<kBrickNT>), to_dim3(bg.grid), block, 0, b->stream,
                           d_params, d_poses, b->d_group_map, b->d_brick_class);
#ifdef TSDF_EXPERIMENTS
    } else if (classify) {   // variant 11: a class per 1024-voxel workgroup patch (round 2a's shape)
        const size_t n_wg = (size_t)b->max_blocks * b->total_slices;
        hipLaunchKernelGGL(tsdfk::classify_workgroups_batched, dim3((unsigned)((n_wg + 255) / 256)), dim3(256), 0, b->stream,
                           d_params, d_poses, b->d_slice_map, b->d_wg_class, b->max_blocks, b->total_slices);
        hipLaunchKernelGGL((tsdfk::integrate_multi_batched_cls<true, true>), grid, block, 0, b->stream, d_params, d_poses,
                           b->d_slice_map, b->d_wg_class);
#endif
    } else {
        hipLaunchKernelGGL((tsdfk::integrate_multi_batched<true>), grid, block, 0, b->stream, d_params, d_poses,
                           b->d_slice_map);
    }
    HIP_TRY(hipGetLastError());
    HIP_TRY(b->blocks.consumed(s, b->stream));
    return TSDF_OK;
}

}  // extern "C"
