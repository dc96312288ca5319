// tsdf_raycast_host.hip.h -- host side of raycasting (tsdf_raycast*, tsdf_batch_raycast_device; tsdf_raycast.hip.h states the rule),
// included at the end of tsdf_capi.hip.  Tracking and association render through its helpers; segmentation shares its camera checks.
#pragma once

namespace {

// An image the 16 x 16 pixel workgroups of the render and the segmenter can cover ...
int image_ok(const char *who, int32_t h, int32_t w)
{
    if (h <= 0 || w <= 0 || (h + 15) / 16 > 65535 || (int64_t)h * w > (int64_t)1 << 30)
        return fail(TSDF_ERR_INVALID, "%s: bad image size %dx%d", who, h, w);
    return TSDF_OK;
}

// ... and a camera over it: what tsdf_raycast_params and tsdf_segment_params have in common.
int camera_ok(const char *who, const float cam_K[9], int32_t h, int32_t w, float near_m, float far_m)
{
    for (int i = 0; i < 9; ++i)
        if (!std::isfinite(cam_K[i])) return fail(TSDF_ERR_INVALID, "%s: cam_K[%d] is not finite", who, i);
    if (cam_K[0] == 0.0f || cam_K[4] == 0.0f) return fail(TSDF_ERR_INVALID, "%s: fx and fy must be non-zero", who);
    int rc = image_ok(who, h, w);
    if (rc) return rc;
    if (!std::isfinite(near_m) || !std::isfinite(far_m) || !(near_m >= 0.0f) || !(near_m < far_m))
        return fail(TSDF_ERR_INVALID, "%s: need 0 <= near < far, both finite (near %g, far %g)", who, (double)near_m, (double)far_m);
    return TSDF_OK;
}

int ray_params_ok(const char *who, const tsdf_raycast_params *p)
{
    if (!p) return fail(TSDF_ERR_INVALID, "%s: NULL parameters", who);
    return camera_ok(who, p->cam_K, p->im_height, p->im_width, p->near_m, p->far_m);
}

int ray_volume_ok(const char *who, const tsdf_volume *v)
{
    const tsdf_config &c = v->cfg;
    if (c.z_begin != 0 || c.z_end != c.dim_z)
        return fail(TSDF_ERR_INVALID, "%s: the handle is the z-slab [%d,%d) of %d slices; raycasting needs a whole-grid handle",
                    who, c.z_begin, c.z_end, c.dim_z);
    if (c.dim_x < 2 || c.dim_y < 2 || c.dim_z < 2)
        return fail(TSDF_ERR_INVALID, "%s: every dim must be >= 2 (%d,%d,%d)", who, c.dim_x, c.dim_y, c.dim_z);
    return TSDF_OK;
}

// The volume as the march sees it, under the relative pose c2b (host float32 arithmetic: go and s_free are part of the rule).
tsdfk::RayVolume ray_volume(const tsdf_volume *v, const float c2b[16])
{
    const tsdf_config &c = v->cfg;
    tsdfk::RayVolume V;
    V.tsdf = v->d_tsdf;
    V.weight = v->d_weight;
    const int dims[3] = {c.dim_x, c.dim_y, c.dim_z};
    for (int i = 0; i < 3; ++i) {
        for (int j = 0; j < 3; ++j) V.r[3 * i + j] = c2b[4 * i + j];
        V.go[i] = (c2b[4 * i + 3] - c.origin[i]) / c.voxel_size;
        V.hi[i] = (float)(dims[i] - 1);
        V.dim[i] = dims[i];
    }
    V.vs = c.voxel_size;
    V.s_free = 0.8f * c.trunc_margin;
    V.max_steps = (int)std::min<int64_t>(2 * ((int64_t)c.dim_x + c.dim_y + c.dim_z) + 8, INT32_MAX);
    return V;
}

template <typename P>
void ray_camera(P &k, const tsdf_raycast_params *p)
{
    k.fx = p->cam_K[0]; k.fy = p->cam_K[4]; k.cx = p->cam_K[2]; k.cy = p->cam_K[5];
    k.near_m = p->near_m; k.far_m = p->far_m; k.wthr = p->weight_thresh;
    k.H = p->im_height; k.W = p->im_width;
}

dim3 ray_grid(const tsdf_raycast_params *p) { return dim3((p->im_width + 15) / 16, (p->im_height + 15) / 16); }

int raycast_checks(const char *who, tsdf_volume *v, const tsdf_raycast_params *p, const float *cam2world, bool any_out,
                          bool want_label, bool want_colour)
{
    if (!v || !cam2world) return fail(TSDF_ERR_INVALID, "%s: NULL argument", who);
    if (!any_out) return fail(TSDF_ERR_INVALID, "%s: every output is NULL", who);
    int rc = ray_params_ok(who, p);
    if (rc == TSDF_OK) rc = ray_volume_ok(who, v);
    if (rc) return rc;
    if (want_label && !v->d_label) return fail(TSDF_ERR_INVALID, "%s: a label image needs tsdf_labels_enable", who);
    if (want_colour && !v->d_colour) return fail(TSDF_ERR_INVALID, "%s: a colour image needs tsdf_colour_enable", who);
    return bind_device(v);   // the collected frames first
}

int launch_raycast(tsdf_volume *v, const tsdf_raycast_params *p, const float cam2world[16], float *depth, float *normal,
                          uint16_t *label, uint32_t *colour)
{
    float c2b[16];
    compose_cam2base(v, cam2world, c2b);
    tsdfk::RaycastParams k;
    k.vol = ray_volume(v, c2b);
    k.label = v->d_label; k.colour = v->d_colour;
    k.depth = depth; k.normal = normal; k.label_out = label; k.colour_out = colour;
    ray_camera(k, p);
    hipLaunchKernelGGL(tsdfk::raycast_volume, ray_grid(p), dim3(256), 0, v->stream, k);
    HIP_TRY(hipGetLastError());
    return TSDF_OK;
}

// The checks of a batch render, then the members' collected frames.
int batch_render_checks(const char *who, tsdf_batch *b, const tsdf_raycast_params *p)
{
    int rc = ray_params_ok(who, p);
    for (size_t i = 0; i < b->vols.size() && rc == TSDF_OK; ++i) rc = ray_volume_ok(who, b->vols[i]);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(b->device));
    for (tsdf_volume *v : b->vols) {   // the batch's collected frames, then any a member collected through its own handle
        rc = bind_device(v);
        if (rc) return rc;
    }
    return TSDF_OK;
}

// Every member into one image, queued on the batch's stream.
int batch_render(tsdf_batch *b, const tsdf_raycast_params *p, const float cam2world[16], float *depth_dev,
                        float *normal_dev, int32_t *member_dev)
{
    const int n = (int)b->vols.size();
    decltype(b->ray)::Slot *s = nullptr;
    HIP_TRY(b->ray.take(&s));
    if (!s->dev) HIP_TRY(staged_alloc(*s, s->done, n * sizeof(tsdfk::RayVolume)));
    for (int i = 0; i < n; ++i) {
        float c2b[16];
        compose_cam2base(b->vols[i], cam2world, c2b);   // each object has its own base frame (ref: src/Object.cpp:23-29)
        s->host[i] = ray_volume(b->vols[i], c2b);
    }
    HIP_TRY(hipMemcpyAsync(s->dev, s->host, n * sizeof(tsdfk::RayVolume), hipMemcpyHostToDevice, b->stream));
    HIP_TRY(b->ray.consumed(s, b->stream));
    tsdfk::BatchRaycastParams k;
    k.members = s->dev;
    k.n = n;
    k.depth = depth_dev; k.normal = normal_dev; k.member = member_dev;
    ray_camera(k, p);
    hipLaunchKernelGGL(tsdfk::raycast_batch, ray_grid(p), dim3(256), 0, b->stream, k);
    HIP_TRY(hipGetLastError());
    return TSDF_OK;
}

}  // namespace

extern "C" {

int tsdf_raycast_params_default(const tsdf_config *cfg, tsdf_raycast_params *out)
{
    if (!cfg || !out) return fail(TSDF_ERR_INVALID, "tsdf_raycast_params_default: NULL argument");
    std::memcpy(out->cam_K, cfg->cam_K, sizeof out->cam_K);
    out->im_height = cfg->im_height;
    out->im_width = cfg->im_width;
    out->near_m = 0.0f;
    out->far_m = cfg->max_depth;
    out->weight_thresh = 0.9f;
    return TSDF_OK;
}

int tsdf_raycast_device(tsdf_volume *v, const tsdf_raycast_params *p, const float cam2world[16], float *depth_dev,
                        float *normal_dev, uint16_t *label_dev, uint32_t *colour_dev)
{
    int rc = raycast_checks("tsdf_raycast_device", v, p, cam2world, depth_dev || normal_dev || label_dev || colour_dev,
                            label_dev != nullptr, colour_dev != nullptr);
    if (rc) return rc;
    return launch_raycast(v, p, cam2world, depth_dev, normal_dev, label_dev, colour_dev);
}

int tsdf_raycast(tsdf_volume *v, const tsdf_raycast_params *p, const float cam2world[16], float *depth_host,
                 float *normal_host, uint16_t *label_host, uint32_t *colour_host)
{
    int rc = raycast_checks("tsdf_raycast", v, p, cam2world, depth_host || normal_host || label_host || colour_host,
                            label_host != nullptr, colour_host != nullptr);
    if (rc) return rc;
    // the images go through the handle's output list buffer (kept between calls), one copy each, then one wait
    const size_t px = (size_t)p->im_height * p->im_width;
    tsdf_host::Regions r;
    const size_t o_d = r.add(px * 4), o_n = r.add(px * 12), o_l = r.add(px * 2), o_c = r.add(px * 4);
    HIP_TRY(v->d_list.ensure(r.total()));
    char *base = v->d_list;
    float *d = depth_host ? reinterpret_cast<float *>(base + o_d) : nullptr;
    float *n = normal_host ? reinterpret_cast<float *>(base + o_n) : nullptr;
    uint16_t *l = label_host ? reinterpret_cast<uint16_t *>(base + o_l) : nullptr;
    uint32_t *c = colour_host ? reinterpret_cast<uint32_t *>(base + o_c) : nullptr;
    rc = launch_raycast(v, p, cam2world, d, n, l, c);
    if (rc) return rc;
    if (d) HIP_TRY(hipMemcpyAsync(depth_host, d, px * 4, hipMemcpyDeviceToHost, v->stream));
    if (n) HIP_TRY(hipMemcpyAsync(normal_host, n, px * 12, hipMemcpyDeviceToHost, v->stream));
    if (l) HIP_TRY(hipMemcpyAsync(label_host, l, px * 2, hipMemcpyDeviceToHost, v->stream));
    if (c) HIP_TRY(hipMemcpyAsync(colour_host, c, px * 4, hipMemcpyDeviceToHost, v->stream));
    HIP_TRY(hipStreamSynchronize(v->stream));
    return TSDF_OK;
}

int tsdf_batch_raycast_device(tsdf_batch *b, const tsdf_raycast_params *p, const float cam2world[16], float *depth_dev,
                              float *normal_dev, int32_t *member_dev)
{
    const char *who = "tsdf_batch_raycast_device";
    if (!b || !cam2world) return fail(TSDF_ERR_INVALID, "%s: NULL argument", who);
    if (!depth_dev && !normal_dev && !member_dev) return fail(TSDF_ERR_INVALID, "%s: every output is NULL", who);
    int rc = batch_render_checks(who, b, p);
    if (rc) return rc;
    return batch_render(b, p, cam2world, depth_dev, normal_dev, member_dev);
}

}  // extern "C"
