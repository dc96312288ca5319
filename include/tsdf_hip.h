/*
 * tsdf_hip.h -- C ABI of libtsdf_hip.so, the MI355X (gfx950) TSDF volumetric-fusion library.
 *
 * This is the drop-in boundary for the dense-grid TSDF path of Tariq-Abuhashim/semantic-slam.
 * Every entry point below replaces one piece of the reference's `class TSDF`
 * (include/tsdf.hpp:22-98, src/tsdf.cu) and is what a binding on the reference side would
 * call (include/tsdf.hpp and include/TSDFfusion.hpp in this repository
 * are those bindings for C++).  Citations "ref:" are paths inside the reference repository.
 * The library's measurement and tuning aids (timers, probes, self-tests, statistics, knobs) are declared apart, in
 * tsdf_hip_diag.h; they are not part of this contract.
 *
 * Conventions
 *   - plain C: opaque handle, pointers and sizes only; no C++/torch types cross the boundary
 *   - every function returns TSDF_OK (0) or a negative tsdf_status; the message of the last
 *     failure on the calling thread is tsdf_last_error()
 *   - matrices are 16 floats, row-major 4x4 (ref: src/tsdf.cu:253); intrinsics are 9 floats,
 *     row-major 3x3 (ref: include/tsdf.hpp:96)
 *   - grids are x-fastest: index = (z*dim_y + y)*dim_x + x (ref: src/tsdf.cu:52)
 *   - a handle owns one z-slab [z_begin, z_end) of the global grid on one device and one
 *     HIP stream; distinct handles may be driven from distinct threads, one handle may not
 *     (ref: the reference holds one TSDF per Object and never shares it, src/Engine.cpp:170-172)
 *   - "host" pointers are ordinary memory the caller owns and may free as soon as the call
 *     returns; "device" pointers are HBM addresses valid on the handle's device
 *   - a caller's device pointer (every *_dev argument: depth, mask, rgb, raw, label, score, member, render, cluster and halo
 *     images, in and out) needs the alignment of its element type only -- 4 bytes for float / int32 / uint32, 2 for uint16,
 *     none for bytes -- so a sub-buffer of a frame ring or an image ROI may be passed as it is.  Exactly the stated number
 *     of elements is read, or written, and nothing outside them: not a byte before the first element or after the last, not
 *     even a load whose value is discarded.  Where a kernel takes a wider access it chooses it at run time from the
 *     pointer's low bits and the image size and falls back to element accesses otherwise (DESIGN.md lists which;
 *     tests/test_gpu_caller_buffers.py holds every such entry point to this between guard bands)
 */
#ifndef TSDF_HIP_H
#define TSDF_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct tsdf_volume tsdf_volume; /* opaque */

typedef enum tsdf_status {
    TSDF_OK = 0,
    TSDF_ERR_INVALID = -1,   /* bad argument (NULL, non-positive size, slab outside the grid) */
    TSDF_ERR_HIP = -2,       /* a HIP runtime call failed; tsdf_last_error() has its name */
    TSDF_ERR_IO = -3,        /* file could not be written / read */
    TSDF_ERR_NO_DEVICE = -4  /* no usable gfx950 device */
} tsdf_status;

/*
 * Everything that is a compile-time member initialiser in the reference, made run-time.
 * tsdf_config_default() fills in exactly the reference's values:
 *   dims 200^3, voxel 0.004 m, trunc 5*voxel   (ref: include/tsdf.hpp:63-67)
 *   K = TUM fr3 {535.4,0,320.1, 0,539.2,247.6, 0,0,1} (ref: include/tsdf.hpp:96)
 *   max_depth 6 m                               (ref: src/tsdf.cu:46)
 *   base2world = identity, origin = 0, slab = whole grid, device 0
 */
typedef struct tsdf_config {
    int32_t im_height, im_width;       /* depth image size (ref ctor args h, w: src/tsdf.cu:62) */
    int32_t dim_x, dim_y, dim_z;       /* GLOBAL grid size in voxels */
    int32_t z_begin, z_end;            /* this handle's slab, global z in [z_begin, z_end) */
    float voxel_size;                  /* metres */
    float trunc_margin;                /* metres */
    float max_depth;                   /* depth samples > max_depth are ignored */
    float origin[3];                   /* grid origin in the base camera frame (ref ctor arg) */
    float cam_K[9];                    /* intrinsics */
    float base2world[16];              /* base camera pose (ref ctor arg base2world_vec) */
    int32_t device;                    /* HIP device ordinal */
    int32_t id;                        /* names tsdf<id>.ply / tsdf<id>.bin (ref: src/tsdf.cu:109,116) */
} tsdf_config;

/* Fill *cfg with the reference defaults for an h x w depth image. */
int tsdf_config_default(tsdf_config *cfg, int32_t im_height, int32_t im_width);

/*
 * Replaces TSDF::TSDF (ref: src/tsdf.cu:62-96): allocates the slab in HBM, sets TSDF = 1 and
 * weight = 0 on the device (no host fill + upload), inverts base2world (a singular
 * base2world leaves the inverse all-zero and is not an error, as in ref: src/tsdf.cu:74).
 */
int tsdf_create(const tsdf_config *cfg, tsdf_volume **out);

/* Frees device memory, the stream and staging buffers.  Writes no files (see tsdf_save_*). */
int tsdf_destroy(tsdf_volume *vol);

/* Back to TSDF = 1, weight = 0 (ref: src/tsdf.cu:79-81), asynchronously on the handle's stream. */
int tsdf_reset(tsdf_volume *vol);

/*
 * Replaces TSDF::Integrate (ref: src/tsdf.cu:135-168).  depth_host: im_height*im_width floats,
 * metres, row-major, borrowed for the call only (copied to a pinned staging slot before
 * returning).  cam2world: current camera pose.  cam2base = inverse(base2world) * cam2world
 * is composed on the host in the reference's fp32 operation order (ref: src/tsdf.cu:142).
 * The call does not wait for the GPU.  DEFERRED INTEGRATION: the reference never reads a result back before its
 * destructor (ref: src/tsdf.cu:101-104), so the frames of successive calls are collected in HBM and applied 32 at a
 * time as one fused sequence (tsdf_integrate_frames_device: same results, bit for bit, several times the throughput);
 * every entry point that observes or changes the volume -- sync, download, extraction, save, reset, any other integrate
 * call -- first applies what has been collected.  tsdf_set_deferral(vol, 0) makes every call launch its own kernel.
 */
int tsdf_integrate(tsdf_volume *vol, const float *depth_host, const float cam2world[16]);
/* Frames tsdf_integrate collects per launch: 0 or 1 = none (one kernel per call), at most 32 (the default). */
int tsdf_set_deferral(tsdf_volume *vol, int32_t n_frames);

/*
 * Same from the sensor's raw 16-bit frame (TUM PNG payload): copies im_height*im_width uint16
 * (half the bytes of the float frame), converts on the device to metres with
 * value * (1.0f / depth_factor), keeping only pixels with row % row_step == 0 and
 * col % col_step == 0 (others become 0), then integrates.  depth_factor 5000, steps (4, 3)
 * reproduce the offline labeller's preparation (ref: examples/label_instance_rgbd.cpp:89-100,
 * config/TUM3.yaml:34); steps (1, 1) keep the whole frame.
 */
int tsdf_integrate_u16(tsdf_volume *vol, const uint16_t *raw_host, float depth_factor, int32_t row_step,
                       int32_t col_step, const float cam2world[16]);

/* The conversion alone, device to device, queued on the handle's stream. */
int tsdf_convert_depth_u16(tsdf_volume *vol, const uint16_t *raw_dev, float *depth_dev, float depth_factor,
                           int32_t row_step, int32_t col_step);

/*
 * Same, with the depth frame already resident in HBM on the handle's device.  Deferred like tsdf_integrate: the frame is
 * copied device to device into the collecting pool on the handle's stream (the ordering its kernel would have had), so
 * depth_dev may be reused under that stream's order as before; with deferral off the kernel reads depth_dev itself.
 * tsdf_integrate_cam2base and tsdf_integrate_masked_device (mask copied with the frame) are collected the same way.
 */
int tsdf_integrate_device(tsdf_volume *vol, const float *depth_dev, const float cam2world[16]);

/*
 * Same as tsdf_integrate_device, for callers that composed the relative pose themselves
 * (cam2base is used as given; base2world is ignored).
 */
int tsdf_integrate_cam2base(tsdf_volume *vol, const float *depth_dev, const float cam2base[16]);

/*
 * A known sequence of frames (offline replay of saved keyframes, ref:
 * examples/label_instance_rgbd.cpp:78-110): exactly n_frames consecutive tsdf_integrate_device /
 * tsdf_integrate_masked_device calls -- same results, bit for bit -- but the library may apply
 * several frames per pass over the volume (weights read and written once per group).
 * depth_dev: n_frames device pointers; masks_dev: NULL or n_frames device pointers (entries may be
 * NULL); cam2world: n_frames x 16 floats.
 * Ordering: every frame (and mask) must be readable once the work queued on the handle's stream before this call has
 * run, and must stay unchanged until the work queued by this call has run.  On slabs below 64 M voxels the library
 * reads the frames of a later pass (their depth tile tables, the brick work list) on a side stream of its own while an
 * earlier pass is still integrating; that stream waits for an event recorded on the handle's stream when the call starts
 * and is joined to the handle's stream before the call returns, so the caller sees one stream as before.
 */
int tsdf_integrate_frames_device(tsdf_volume *vol, const float *const *depth_dev, const uint8_t *const *masks_dev,
                                 const float *cam2world, int32_t n_frames);

/*
 * Per-instance fusion as the reference's caller prepares it: depth * (mask/255) with an
 * 8-bit {0,255} instance mask (ref: src/Engine.cpp:192-193), fused into the depth load
 * instead of materialising the masked image.  mask_dev: im_height*im_width bytes in HBM.
 */
int tsdf_integrate_masked_device(tsdf_volume *vol, const float *depth_dev, const uint8_t *mask_dev,
                                 const float cam2world[16]);

/* Block until everything queued on the handle's stream has finished. */
int tsdf_sync(tsdf_volume *vol);

/*
 * Copy this handle's slab to host arrays of tsdf_slab_voxels() floats each (either may be
 * NULL).  The reference only ever reads results back in its destructor
 * (ref: src/tsdf.cu:101-104); this is the same copy, callable at any time.  Synchronous.
 */
int tsdf_download(tsdf_volume *vol, float *tsdf_host, float *weight_host);

/*
 * Copy n_slices whole z-slices starting at slab-local slice z_local into tsdf_dst / weight_dst
 * (either may be NULL), each n_slices*dim_y*dim_x floats.  The destinations may be host or
 * device addresses (the copy kind is inferred), so a one-slice halo can go straight into a
 * communication buffer in HBM.  Synchronous with respect to the handle's stream.
 */
int tsdf_copy_slices(tsdf_volume *vol, int32_t z_local, int32_t n_slices, void *tsdf_dst, void *weight_dst);

/* Restore a slab from host arrays (resume from a saved state).  Synchronous. */
int tsdf_upload(tsdf_volume *vol, const float *tsdf_host, const float *weight_host);

/*
 * Device addresses of the slab's two arrays (x-fastest, slab-local z).  The library keeps a
 * small summary of both arrays (segments whose TSDF values are all 1, segments whose weights are all one
 * count); after WRITING TSDF values OR WEIGHTS through these pointers call
 * tsdf_refresh_summary().  Reading needs nothing.
 */
int tsdf_refresh_summary(tsdf_volume *vol);
int tsdf_device_ptrs(tsdf_volume *vol, float **tsdf_dev, float **weight_dev);

/* Number of voxels in this handle's slab: dim_x * dim_y * (z_end - z_begin). */
int64_t tsdf_slab_voxels(const tsdf_volume *vol);

/* Copy of the configuration the handle was created with. */
int tsdf_get_config(const tsdf_volume *vol, tsdf_config *out);

/*
 * Run subsequent work of this handle on a caller-owned hipStream_t (passed as void*), e.g.
 * the current PyTorch stream, or back on the handle's own stream when stream == NULL.
 * (Copies of host frames run on the store's copy stream and, for sequence calls, table kernels on a side stream of the
 * handle; both are ordered against this stream by events, so work queued on it after a call sees that call's result.)
 */
int tsdf_set_stream(tsdf_volume *vol, void *hip_stream);
int tsdf_get_stream(tsdf_volume *vol, void **hip_stream);

/*
 * Number of voxels whose weight is > weight_thresh and whose TSDF is non-zero: the surface
 * test of ref: src/tsdf.cu:179, counted on the device.  Synchronous.
 */
int tsdf_count_surface(tsdf_volume *vol, float weight_thresh, int64_t *count);

/*
 * Surface points of the slab in grid order, xyz triples in the base camera frame
 * (ref: src/tsdf.cu:195-212), compacted on the device.  xyz_host receives at most
 * capacity points; *count is the number found.  Synchronous.
 */
int tsdf_extract_surface(tsdf_volume *vol, float weight_thresh, float *xyz_host, int64_t capacity,
                         int64_t *count);

/*
 * Zero-crossing surface vertices (the vertex set of marching cubes), compacted on the device in
 * grid order: for every voxel and every +x, +y, +z neighbour with both weights > weight_thresh and
 * TSDF values of opposite sign, the linearly interpolated crossing point.  Not a reference
 * function (its mesh path is the absent tsdf-fusion-python, ref: src/TSDFfusion.py.in:48-53); the
 * rule is defined in oracle/tsdf_oracle.c (oracle_zero_crossings) and csrc/tsdf_extract.hip.h.
 * halo_tsdf / halo_weight: the dim_y*dim_x values of global slice z_end -- what a z-slab owner
 * receives from its upper neighbour (host or device memory) -- or both NULL on the top slab.
 * Call with xyz_host == NULL to get *count only.  Synchronous.
 */
int tsdf_extract_crossings(tsdf_volume *vol, const float *halo_tsdf, const float *halo_weight, float weight_thresh,
                           float *xyz_host, int64_t capacity, int64_t *count);

/*
 * Triangle mesh of the zero level set by marching tetrahedra, on the device, cubes in grid order,
 * 9 floats (3 vertices) per triangle; a watertight, consistently wound triangle soup (edge vertices of
 * neighbouring cubes are bit-identical).  Stands in for the reference's SaveMesh, which needs the absent
 * tsdf-fusion-python (ref: src/TSDFfusion.py.in:48-53); rule in csrc/tsdf_extract.hip.h, checked against
 * this project's CPU restatement only.  halo_* as for tsdf_extract_crossings.  tsdf_save_mesh_ply writes a
 * binary .ply (vertex + face elements) of a whole-grid handle.
 */
int tsdf_extract_mesh(tsdf_volume *vol, const float *halo_tsdf, const float *halo_weight, float weight_thresh,
                      float *triangles_host, int64_t capacity, int64_t *count);
int tsdf_save_mesh_ply(tsdf_volume *vol, const char *path, float weight_thresh);
/*
 * The same mesh as the reference's Python glue saves it (ref: src/TSDFfusion.py.in:48-53, get_mesh -> verts, faces,
 * norms, colors -> meshwrite): shared (welded) vertices -- the soup's edge vertices are bit-identical between cubes, so
 * welding matches coordinate bits exactly --, an area-weighted normal per vertex, a colour per vertex when colour is
 * enabled, faces as vertex indices in the soup's order and winding.  Binary little-endian .ply.
 */
int tsdf_save_mesh_welded_ply(tsdf_volume *vol, const char *path, float weight_thresh);

/*
 * File writers, byte-compatible with the reference's destructor (ref: src/tsdf.cu:107-132,
 * 170-218).  For a slab handle the .bin header carries the slab's dims and a z-shifted
 * origin is NOT applied: callers that shard gather slabs in z order first (see
 * semantic_slam_amd/sharded.py); a whole-grid handle writes exactly the reference's files.
 *   .ply: binary_little_endian points with |tsdf| != 0 and weight > weight_thresh (0.9 in the ref); the reference
 *         prints the vertex count with %d, so more than 2^31 - 1 points cannot be represented: TSDF_ERR_INVALID
 *   .bin: 8-float header {dim_x, dim_y, dim_z, origin xyz, voxel_size, trunc} + TSDF floats
 */
int tsdf_save_ply(tsdf_volume *vol, const char *path, float weight_thresh);
int tsdf_save_bin(tsdf_volume *vol, const char *path);

/*
 * Checkpoint / resume.  The reference only writes (ref: src/tsdf.cu:114-132) and nothing in it reads a
 * .bin back.  tsdf_load_bin restores the TSDF array from a file in the reference's .bin format (its
 * 8-float header must match the slab; weights are not in that format and are left untouched).
 * tsdf_save_state / tsdf_load_state round-trip the whole slab (configuration, TSDF, weights) in this
 * library's own format, so an interrupted fusion continues bit-exactly.
 */
int tsdf_load_bin(tsdf_volume *vol, const char *path);
int tsdf_save_state(tsdf_volume *vol, const char *path);
int tsdf_load_state(tsdf_volume *vol, const char *path);

/*
 * Integrate AND label fusion of a known sequence of frames in the same passes over the volume: identical to
 * calling tsdf_integrate_device and tsdf_integrate_labels_device for every frame in order, but the label
 * evidence reuses the projection and depth tests Integrate has just made (the separate sweep recomputes
 * them).  Needs dim_x % 4 == 0 and tsdf_labels_enable.  All pointers are device pointers that stay valid
 * until the stream has run the launches.
 */
int tsdf_integrate_frames_labels_device(tsdf_volume *vol, const float *const *depth_dev,
                                        const uint16_t *const *label_im_dev, const float *const *score_im_dev,
                                        const float *cam2world, int32_t n_frames);

/*
 * Per-voxel semantic-label fusion (BASELINE config 5).  Not a function of the reference's TSDF:
 * the reference fuses instance evidence per sparse ObjectPoint -- Fp += score inside a mask of the
 * point's object, Bp += score otherwise, P = Fp/(Fp+Bp), dropped below a threshold
 * (ref: src/ObjectPoint.cpp:190-219,149-154; Engine.mProbThd = 0.5, config/TUM3.yaml:92); the same
 * rule is applied here per voxel of the dense grid (csrc/tsdf_labels.hip.h states it exactly).
 *   tsdf_labels_enable        allocate (or clear) label:uint16, Fp:f32, Bp:f32 arrays for the slab
 *   tsdf_compose_labels       K instance masks (MaskRCNN format, ref: src/MaskRCNN.cpp:316-362:
 *                             K*H*W uint8 {0,255} in device memory, label and score per instance on
 *                             the host) -> one label image + one score image on the device
 *   tsdf_integrate_labels_device  one frame: voxels observed inside the truncation band (same pixel
 *                             and depth tests as tsdf_integrate*) take evidence from the label image
 *   tsdf_download_labels      copy the three arrays out (any pointer may be NULL)
 */
int tsdf_labels_enable(tsdf_volume *vol, float prob_threshold);
int tsdf_compose_labels(tsdf_volume *vol, const uint8_t *masks_dev, const uint16_t *labels_host,
                        const float *scores_host, int32_t k, uint16_t *label_im_dev, float *score_im_dev);
int tsdf_integrate_labels_device(tsdf_volume *vol, const float *depth_dev, const uint16_t *label_im_dev,
                                 const float *score_im_dev, const float cam2world[16]);
int tsdf_download_labels(tsdf_volume *vol, uint16_t *label_host, float *fp_host, float *bp_host);

/*
 * Per-voxel colour fusion for the TSDFfusion surface.  The reference's second backend passes every RGB-D frame to the
 * third-party tsdf-fusion-python (ref: src/TSDFfusion.py.in:43 `integrate(color_image, depth_im, cam_intr, cam_pose,
 * obs_weight=1.)`), which fuses colour beside the distance and colours its mesh (ref: src/TSDFfusion.py.in:48-53).  That
 * package is absent, so this restates its published rule (csrc/tsdf_colour.hip.h): every voxel a frame updates takes per
 * 8-bit channel min(255, round((c * w_old + c_pixel) / w_new)); parity unpinned.
 *   tsdf_colour_enable            allocate (or clear) one packed colour (0x00BBGGRR) per voxel of the slab
 *   tsdf_integrate_colour_device  the colour pass of ONE frame, to be queued right after that frame's
 *                                 tsdf_integrate*_device call (it reads the weights that call has written);
 *                                 rgb_dev: im_height*im_width*3 bytes, channel 0 = R
 *   tsdf_integrate_rgbd           both passes from host images (TSDFfusion::Integrate): copies depth and colour to
 *                                 pinned staging, integrates, then fuses colour; the call does not wait
 *   tsdf_download_colour          copy the packed colours out (tsdf_slab_voxels() uint32)
 * With colour enabled tsdf_save_mesh_ply writes per-vertex red/green/blue (the nearest voxel's colour).
 * The colour pass has no weight of its own: it takes w_new from the weight array the geometry pass has just written and
 * w_old = w_new - 1 (the package's obs_weight = 1).  So (i) a frame integrated WITHOUT a colour image (tsdf_integrate*, or
 * TSDFfusion::Integrate with an empty colour Mat) still raises the weight, and later colour frames are blended as if that
 * frame had confirmed the colour the voxel already had -- the behaviour of the package when every frame brings colour, a
 * documented deviation otherwise; (ii) past 2^24 updates of one voxel w_new - 1 is no longer exact in fp32 (the weights
 * themselves stop counting there, as the reference's do).  The pass re-derives the frame's updated voxels with the same
 * projection code as Integrate; tests/test_gpu_colour.py checks the two sets voxel for voxel on poses that send wavefronts of
 * both kernels down the generic projection.
 */
int tsdf_colour_enable(tsdf_volume *vol);
int tsdf_integrate_colour_device(tsdf_volume *vol, const float *depth_dev, const uint8_t *rgb_dev,
                                 const float cam2world[16]);
int tsdf_integrate_rgbd(tsdf_volume *vol, const float *depth_host, const uint8_t *rgb_host, const float cam2world[16]);
int tsdf_download_colour(tsdf_volume *vol, uint32_t *colour_host);

/*
 * Raycasting: what the fused model looks like from a camera -- per pixel the depth of the first zero crossing of the TSDF
 * along the pixel's ray, the surface normal there (camera frame, toward the camera), and the fused label and colour of the
 * voxel nearest to it.  Not a reference function (its front end asks this of sparse ObjectPoints, ref: src/Engine.cpp:356-496);
 * the rule is stated exactly in csrc/tsdf_raycast.hip.h and restated in tests/raycast_spec.py.  A miss gives depth 0,
 * normal (0, 0, 0), label 0, colour 0.  Every call applies the handle's (or batch's) collected frames first and reads the
 * volume only: the TSDF, the weights, the summary words, labels and colours are not written.  Whole-grid handles only (a
 * z-slab or a tsdf_group is refused); every dim must be >= 2.
 *   near_m, far_m      0 <= near < far, both finite: the camera-depth range the ray is marched over
 *   weight_thresh      a voxel counts as observed when its weight is > this
 * tsdf_raycast_params_default: the config's K and image size, near 0, far = max_depth, weight_thresh 0.9 (the extraction
 * default).  Host arithmetic only: needs no device.
 */
typedef struct tsdf_raycast_params {
    float cam_K[9];            /* row-major 3x3 */
    int32_t im_height, im_width;
    float near_m, far_m;
    float weight_thresh;
} tsdf_raycast_params;

int tsdf_raycast_params_default(const tsdf_config *cfg, tsdf_raycast_params *out);
/*
 * Device outputs, each may be NULL but not all: depth H*W floats (camera z, metres), normal H*W*3 floats, label H*W uint16
 * (needs tsdf_labels_enable), colour H*W uint32 (needs tsdf_colour_enable).  Queued on the handle's stream (tsdf_set_stream).
 */
int tsdf_raycast_device(tsdf_volume *vol, const tsdf_raycast_params *p, const float cam2world[16], float *depth_dev,
                        float *normal_dev, uint16_t *label_dev, uint32_t *colour_dev);
/* The same into host memory; returns when the images are there. */
int tsdf_raycast(tsdf_volume *vol, const tsdf_raycast_params *p, const float cam2world[16], float *depth_host,
                 float *normal_host, uint16_t *label_host, uint32_t *colour_host);

/*
 * Tracking: the camera pose of a live depth frame, by point-to-plane ICP against the model's raycast (frame-to-model, as in
 * KinectFusion).  Not a reference function (its front end takes poses from ORB-SLAM2, ref: result/rgbd/bundle.txt, and tracks
 * objects through sparse ObjectPoints, ref: src/Engine.cpp:374,550); the rule is stated exactly in csrc/tsdf_track.hip.h and
 * restated in tests/track_spec.py.  On a batch member's borrowed handle with that object's instance mask it tracks the camera
 * against one object's model.
 *   ray                the model render (tsdf_raycast rule): K and image size (= the live frame's), near_m, far_m,
 *                      weight_thresh; near_m < d <= far_m is also the live frame's valid depth range
 *   n_levels           1..3; level l uses every 2^l-th pixel of every 2^l-th row of the live frame
 *   iters[l]           Gauss-Newton iterations of level l (>= 0; 0 skips it); the coarsest level runs first
 *   dist_thresh[l]     metres (finite, > 0): a pair further apart than this is rejected
 *   cos_normal_thresh  in [-1, 1]: a pair whose normals' cosine is below this is rejected
 *   min_inliers        >= 0: an iteration with fewer pairs loses the track
 *   eps_rot, eps_trans finite, > 0: an update with |omega| < eps_rot (rad) and |tau| < eps_trans (m) ends its level
 * tsdf_track_params_default: tsdf_raycast_params_default(cfg); 3 levels; iterations {10, 5, 4}; 0.10 m at every level;
 * cos(20 deg); min_inliers 300 (the coarsest level of a 640x480 frame has 18,921 samples: an object on 5 % of the image
 * gives about 950 of them, 300 leaves room for two thirds of those to be lost at its edges or to the thresholds); eps 1e-5 rad
 * and 1e-5 m.  Host arithmetic only: needs no device.
 */
typedef struct tsdf_track_params {
    tsdf_raycast_params ray;
    int32_t n_levels;
    int32_t iters[3];
    float dist_thresh[3];
    float cos_normal_thresh;
    int32_t min_inliers;
    float eps_rot, eps_trans;
} tsdf_track_params;

typedef struct tsdf_track_result {
    float cam2world[16];       /* the estimate; the guess's own bits when lost */
    int32_t status;            /* 0 converged, 1 iterations exhausted, 2 lost (too few pairs, or a failed Cholesky) */
    int32_t iters_run[3];      /* per level */
    int32_t inliers;           /* pairs of the last iteration run */
    float rmse;                /* sqrt(sum r^2 / inliers) of that iteration, metres */
} tsdf_track_result;

int tsdf_track_params_default(const tsdf_config *cfg, tsdf_track_params *out);
/*
 * depth_dev: the live frame, ray.im_height x ray.im_width floats (metres); mask_dev: as many {0, 255} bytes, or NULL.  Applies
 * the handle's (or its batch's) collected frames, renders the model once at the guess, runs the iterations and returns when
 * the result is on the host; everything is queued on the handle's stream (tsdf_set_stream ordering holds).  Reads the volume
 * only.  Lost is not an error: TSDF_OK with status 2.  Whole-grid handles only (a z-slab or a tsdf_group slab is refused).
 */
int tsdf_track(tsdf_volume *vol, const tsdf_track_params *p, const float *depth_dev, const uint8_t *mask_dev,
               const float guess_cam2world[16], tsdf_track_result *out);
/*
 * The linear system of one iteration of level `level` (0 <= level < n_levels): the model rendered at ref_cam2world, the live
 * frame's pairs at cam2world.  system_out: the 21 upper-triangle entries of J^T J (row-major), the 6 of J^T r, sum r^2, the
 * pair count.  For callers that combine the dense term with residuals of their own.  Returns when the system is on the host.
 */
int tsdf_track_system(tsdf_volume *vol, const tsdf_track_params *p, const float *depth_dev, const uint8_t *mask_dev,
                      const float ref_cam2world[16], const float cam2world[16], int32_t level, double system_out[29]);

/*
 * Photometric tracking: tsdf_track's geometric system plus an intensity residual of the live RGB image against the colour
 * fused into the volume (tsdf_colour_enable), so that a scene whose geometry leaves directions free -- a camera facing a wall
 * -- is still constrained by its texture.  The rule is stated exactly in csrc/tsdf_photo.hip.h and restated in
 * tests/photo_spec.py: per level, A = A_geo + photo_weight^2 * A_photo and b likewise, then tsdf_track's solve and step.
 *   photo_weight       finite, >= 0: metres of point-to-plane residual one unit of intensity ([0, 1]) counts for; 0 = geometric only
 *   intensity_thresh   finite, > 0: a photometric pair whose |residual| exceeds this is rejected
 * tsdf_photo_params_default: photo_weight 0.1, intensity_thresh 0.25.  Host arithmetic only: needs no device.
 * A track is lost as tsdf_track's is, by the GEOMETRIC pair count or a failed pivot of the combined system.
 */
typedef struct tsdf_photo_params {
    float photo_weight;
    float intensity_thresh;
} tsdf_photo_params;

typedef struct tsdf_track_rgbd_result {
    tsdf_track_result geo;     /* as tsdf_track's: inliers and rmse are the geometric pairs' */
    int32_t photo_pairs;       /* photometric pairs of the last iteration run (0 without an rgb image or weight) */
    float photo_rmse;          /* sqrt(sum r^2 / photo_pairs) of that iteration, intensity units */
} tsdf_track_rgbd_result;

int tsdf_photo_params_default(const tsdf_config *cfg, tsdf_photo_params *out);
/*
 * The images are host memory: depth_host ray.im_height x ray.im_width floats (metres), rgb_host as many R, G, B byte triples
 * or NULL, mask_host as many {0, 255} bytes or NULL; each is copied once.  Applies the handle's collected frames first, reads
 * the volume only, and returns when the result is on the host.  With rgb_host NULL or photo_weight 0 it is the geometric
 * track: `geo` is tsdf_track's result on the same frame bit for bit and photo_pairs is 0.  An rgb image needs a handle with
 * colour enabled.  Lost is not an error: TSDF_OK with status 2.  Whole-grid handles only.
 */
int tsdf_track_rgbd(tsdf_volume *vol, const tsdf_track_params *p, const tsdf_photo_params *pp, const float *depth_host,
                    const uint8_t *rgb_host, const uint8_t *mask_host, const float guess_cam2world[16],
                    tsdf_track_rgbd_result *out);
/*
 * Both linear systems of one iteration of level `level`, each in tsdf_track_system's layout, unweighted and not added:
 * geo_out equals tsdf_track_system's output, photo_out is the photometric one.  rgb_host is required.  Returns when both are
 * on the host.
 */
int tsdf_track_rgbd_system(tsdf_volume *vol, const tsdf_track_params *p, const tsdf_photo_params *pp, const float *depth_host,
                           const uint8_t *rgb_host, const uint8_t *mask_host, const float ref_cam2world[16],
                           const float cam2world[16], int32_t level, double geo_out[29], double photo_out[29]);
/*
 * The model intensity image of pyramid level `level` (0..2) seen from cam2world: (im_height >> level) x (im_width >> level)
 * floats in [0, 1], -1 where the model has none.  Trilinear in the fused colours' luminance at the depth render's hit point, so
 * unlike tsdf_raycast's colour output it has a usable image gradient.  For callers who bring residuals of their own.  Returns
 * when the image is on the host.
 */
int tsdf_render_intensity(tsdf_volume *vol, const tsdf_raycast_params *p, const float cam2world[16], int32_t level,
                          float *intensity_host);

/*
 * Merging and re-gridding: every voxel of dst samples src at its own position (trilinear, through both handles' base2world,
 * origin and voxel size) and folds the sample in as one observation whose weight is the smallest of the 8 corner weights.  Two
 * uses: a duplicate object (tsdf_batch_associate answered -1 for a partial view, so one physical object lives in two volumes)
 * is first compared with write = 0 and then merged with write = 1; an object that has outgrown the grid placed from its first
 * frame (tsdf_object_origin) is resampled into a fresh handle with another origin, size or voxel size.  Not a reference
 * function (ref: src/Object.cpp:37-49 places an object's grid once and never moves it); the rule is stated exactly in
 * csrc/tsdf_fuse.hip.h and restated in tests/fuse_spec.py.
 *   weight_thresh   finite: a source corner counts as observed when its weight is > this; a sample needs all 8 corners
 *   agree_tol       finite, > 0: two TSDF values (destination truncation units) agree when they differ by at most this
 *   write           1: update dst; 0: a dry run -- the counts only, not one bit of dst is written
 * Counts, over the destination voxels with a valid sample that the band test did not skip (sample * trunc_src / trunc_dst
 * <= -1: skipped, as Integrate skips diff <= -trunc), with dst's values BEFORE the update:
 *   sampled      all of them                       both_band    of both, |dst tsdf| < 1 and |sample| < 1 (near a surface in both)
 *   both         of those, dst weight > thresh     agree_band   of both_band, |dst tsdf - sample| <= agree_tol
 * Whether two volumes show the same object is the caller's decision from agree_band / both_band; the library makes none.
 * Deviation: labels and colours of dst are neither read nor written.  src is only read.  tsdf_fuse_volume_carry (below) is the
 * same merge that also carries them.
 * Results are specified bit for bit (tests/fuse_spec.py), with one exception: where dst already held a NaN, an infinity or a
 * weight that is not positive the update can yield a NaN, and which NaN (sign, payload) is the hardware's choice; such a voxel
 * is specified as "a NaN".  A valid sample is always finite, so a dst of finite values and weights >= 0 never gets one.
 * tsdf_fuse_params_default: weight_thresh 0.9 (the extraction and raycast default), agree_tol 0.4 (two voxels of the default
 * band of 5 voxels: a choice, not a measurement), write 1.  Host arithmetic only: needs no device.
 * tsdf_fuse_volume: dst and src are plain handles or borrowed batch members, whole-grid handles on the same device.  The
 * collected frames of both are applied first (through their batches where they have one); the kernel runs on dst's stream after
 * everything queued on src's stream so far, and src's stream waits for it, so a later write to src cannot overtake the read; after
 * a writing call dst's free-space summary is rebuilt.  Synchronous like tsdf_batch_associate: returns when the counts are on the
 * host.  Refused with TSDF_ERR_INVALID: a NULL dst, src or p; dst == src; a z-slab or a tsdf_group slab on either side; different
 * devices; a weight_thresh that is not finite; an agree_tol that is not finite or not > 0; a write outside {0, 1}.
 */
typedef struct tsdf_fuse_params { float weight_thresh; float agree_tol; int32_t write; } tsdf_fuse_params;
typedef struct tsdf_fuse_counts { uint64_t sampled, both, both_band, agree_band; } tsdf_fuse_counts;
int tsdf_fuse_params_default(const tsdf_config *dst_cfg, tsdf_fuse_params *out);   /* host arithmetic only */
int tsdf_fuse_volume(tsdf_volume *dst, tsdf_volume *src, const tsdf_fuse_params *p, tsdf_fuse_counts *counts /* may be NULL */);

/*
 * Registration of one volume against another, and the merge at a given pose.  tsdf_fuse_volume samples src through
 * M = inverse(base2world_src) * base2world_dst and nothing else, so both base2world must already put the volumes in the same
 * place.  A duplicate object fused from another stretch of the trajectory carries that stretch's drift, and a moved object a
 * stale pose; there the write = 0 comparison reports a low agree_band / both_band.  tsdf_align_volume estimates the rigid motion
 * dst2src that takes dst's base frame to src's from the two signed-distance fields themselves (direct SDF-to-SDF alignment,
 * Gauss-Newton on the TSDF difference over a coarse-to-fine lattice of dst's voxels), and tsdf_fuse_volume_at merges at it.
 * Not a reference function; the rule is stated exactly in csrc/tsdf_align.hip.h and restated in tests/align_spec.py.
 *   weight_thresh   finite: a voxel or a source corner counts as observed when its weight is > this
 *   resid_thresh    finite, > 0: a pair is dropped when the two TSDF values (dst truncation units) differ by more than this
 *   n_levels        1..3; level l takes every 2^l-th voxel of dst per axis; levels run n_levels - 1 .. 0
 *   iters[l]        >= 0 iterations at level l (0 skips the level)
 *   min_pairs       >= 0: fewer pairs in an iteration and the run is lost
 *   eps_rot, eps_trans   finite, > 0: a level ends when a step is below both (radians, metres)
 * Result: dst2src (row-major 4 x 4, last row 0 0 0 1; on a lost run the starting matrix's own bits), status 0 converged,
 * 1 iterations exhausted, 2 lost (too few pairs, or a failed Cholesky pivot; not an error: TSDF_OK), iters_run per level, and
 * the pairs and rmse = sqrt(sum r^2 / pairs) (dst truncation units) of the last iteration run.
 * Limits: a residual exists only where both fields are inside their truncation bands, so the basin is about one truncation
 * distance of surface displacement; the coarse levels subsample, they do not widen it.  A caller with a larger error starts
 * from a better guess, for instance the two centroids of tsdf_extent_metric.  The library decides nothing: whether the result
 * is trusted is the caller's call from pairs, rmse and a following write = 0 merge.  Labels and colours are not read.
 * tsdf_align_params_default: weight_thresh 0.9, resid_thresh 1.0, 2 levels, iters {10, 10, 0}, min_pairs 300, eps 1e-5 rad /
 * 1e-5 m: choices, not measurements.  tsdf_fuse_pose_default: the M tsdf_fuse_volume composes from the two configurations.
 * Both are host arithmetic only and need no device.
 * tsdf_align_volume: guess_dst2src NULL starts from tsdf_fuse_pose_default's matrix; only the first three rows of a pose are
 * read, and they are taken as given (rigidity is the caller's duty).  tsdf_align_system: one pass of level `level` at the given
 * pose in tsdf_track_system's layout (21 of J^T J, 6 of J^T r, sum r^2, the pair count), for callers who combine terms.
 * tsdf_fuse_volume_at: tsdf_fuse_volume with the first three rows of dst2src in place of M; rule, counts, summary rebuild and
 * refusals are unchanged, and with tsdf_fuse_pose_default's matrix it equals tsdf_fuse_volume bit for bit.
 * All three take the handles tsdf_fuse_volume takes and apply the collected frames of both first.  Queued as tsdf_fuse_volume
 * queues its kernel; each returns when the result is on the host.  The align calls read both volumes only: not one bit of
 * either changes.  Refused with TSDF_ERR_INVALID: everything tsdf_fuse_volume refuses about the handles; a src dim < 2; a
 * weight_thresh that is not finite; a resid_thresh that is not finite or not > 0; n_levels outside 1..3; a negative iters[l]
 * or min_pairs; an eps that is not finite or not > 0; a level outside [0, n_levels); a non-finite entry in the first three
 * rows of a given pose; a NULL dst2src where it is not optional.
 */
typedef struct tsdf_align_params { float weight_thresh, resid_thresh; int32_t n_levels; int32_t iters[3];
                                   int32_t min_pairs; float eps_rot, eps_trans; } tsdf_align_params;
typedef struct tsdf_align_result { float dst2src[16]; int32_t status; int32_t iters_run[3]; int32_t pairs; float rmse; } tsdf_align_result;
int tsdf_align_params_default(const tsdf_config *dst_cfg, tsdf_align_params *out);                 /* host arithmetic only */
int tsdf_fuse_pose_default(const tsdf_config *dst_cfg, const tsdf_config *src_cfg, float dst2src[16]); /* the M tsdf_fuse_volume composes; host only */
int tsdf_align_volume(tsdf_volume *dst, tsdf_volume *src, const tsdf_align_params *p,
                      const float guess_dst2src[16] /* may be NULL */, tsdf_align_result *out);
int tsdf_align_system(tsdf_volume *dst, tsdf_volume *src, const tsdf_align_params *p, const float dst2src[16],
                      int32_t level, double system_out[29]);   /* one pass at the given pose, tsdf_track_system's layout */
int tsdf_fuse_volume_at(tsdf_volume *dst, tsdf_volume *src, const tsdf_fuse_params *p, const float dst2src[16],
                        tsdf_fuse_counts *counts /* may be NULL */);

/*
 * The merge that carries colour and labels, and the uploads of both.  tsdf_fuse_volume and tsdf_fuse_volume_at move the TSDF
 * and the weights only: a re-gridded object would come out black and unlabelled, and a merged duplicate would lose the
 * source's votes.  tsdf_fuse_volume_carry does everything those two do -- the TSDF, the weights and the four counts equal
 * tsdf_fuse_volume (dst2src NULL) or tsdf_fuse_volume_at bit for bit, and with carry == 0 the call is that call -- and the
 * destination voxels the merge updates (counts->sampled of them) also take what `carry` names.  The rule is stated exactly in
 * csrc/tsdf_fuse_carry.hip.h and restated in tests/fuse_carry_spec.py.
 *   TSDF_FUSE_CARRY_COLOUR   per 8-bit channel the source's colour, interpolated over the same 8 corners with the same
 *                            fractions, is blended in with the merge's own weights: round((c_dst * w_dst + c_src * w_src) /
 *                            (w_dst + w_src)) clamped to 0..255, with w_dst dst's weight BEFORE the merge and w_src the
 *                            sample's; a voxel with w_dst == 0 takes the interpolated colour itself.  Only with write = 1.
 *   TSDF_FUSE_CARRY_LABELS   the nearest source voxel (per axis the upper corner from a fraction of 0.5) is one observation of
 *                            its label L with score Fp, folded in by tsdf_integrate_labels_device's rule and dst's
 *                            prob_threshold: a source label 0 changes nothing; an unlabelled dst voxel takes (L, Fp, Bp);
 *                            an equal label adds Fp to Fp and Bp to Bp; another label adds the source's Fp to dst's Bp and,
 *                            if Fp / (Fp + Bp) then falls below the threshold, dst takes (L, Fp, Bp).
 * carry_counts, over the updated voxels whose source label is not 0: label_adopted, label_agreed, label_opposed and, of the
 * opposed, label_flipped.  Taken with write = 0 too (not one bit of dst is written then); all zero without the labels bit.
 * tsdf_upload_labels / tsdf_upload_colour mirror tsdf_download_labels / tsdf_download_colour: tsdf_slab_voxels() elements per
 * array, the collected frames applied first, as tsdf_upload does; all pointers are required.
 * tsdf_fuse_volume_carry takes the handles tsdf_fuse_volume takes and applies the collected frames of both first.  Queued as
 * tsdf_fuse_volume queues its kernel; returns when the counts are on the host.  src is only read.  Refused with
 * TSDF_ERR_INVALID: everything tsdf_fuse_volume_at refuses, except that a NULL dst2src means the M tsdf_fuse_volume composes;
 * carry with bits outside 3; colour asked for while colour is not enabled on dst or on src, labels likewise (the message
 * names the side).  The uploads refuse a NULL argument and an attribute that is not enabled.
 * Out of scope: a z-slab or tsdf_group handle on either side; labels and colour in tsdf_save_state; a trilinear or majority
 * label vote; counts of colour agreement.
 */
#define TSDF_FUSE_CARRY_COLOUR 1u
#define TSDF_FUSE_CARRY_LABELS 2u
typedef struct tsdf_fuse_carry_counts { uint64_t label_adopted, label_agreed, label_opposed, label_flipped; } tsdf_fuse_carry_counts;
int tsdf_fuse_volume_carry(tsdf_volume *dst, tsdf_volume *src, const tsdf_fuse_params *p,
                           const float dst2src[16] /* NULL: the M tsdf_fuse_volume composes */, uint32_t carry,
                           tsdf_fuse_counts *counts /* may be NULL */, tsdf_fuse_carry_counts *carry_counts /* may be NULL */);
int tsdf_upload_labels(tsdf_volume *vol, const uint16_t *label_host, const float *fp_host, const float *bp_host);
int tsdf_upload_colour(tsdf_volume *vol, const uint32_t *colour_host);

/*
 * Extent: what a fused volume holds -- how many voxels were observed, how many lie near a surface, where those are (sums,
 * second moments, index bounds) and how many of them sit against each face of the grid.  Three decisions of the per-object
 * loop read it: whether an object has outgrown the grid placed from its first frame (ref: src/Object.cpp:37-49 places it once;
 * tsdf_fuse_volume moves the content, tsdf_extent_regrid proposes where to), whether an instance is worth keeping (the dense
 * counterpart of HasEnoughObjectPoints, ref: src/Object.cpp:305-309, src/Engine.cpp:238-250), and where the object is (ref:
 * src/Engine.cpp:550 matches instances by 2-D contour centroids and asks "should this be the TSDF center instead ?").  Not a
 * reference function; the rule is stated in csrc/tsdf_extent.hip.h and restated with exact integers in tests/extent_spec.py.
 * The library makes none of these decisions.
 *   For the voxel at GLOBAL grid index (x, y, z) with TSDF t and weight w:
 *     observed   w > weight_thresh
 *     surface    observed && fabsf(t) < band      (a NaN t is never surface; a free-space t == 1 is not when band == 1)
 *   The record holds integers only, so it is specified bit for bit and does not depend on the order of the reduction.  A
 *   voxel near two faces counts for both; margin == 0 leaves all six border counts 0.
 *   weight_thresh   finite                 band   finite, in (0, 1]                 margin   >= 0
 * tsdf_extent_params_default: weight_thresh 0.9 (the extraction, raycast and merge default), band 1.0 (anywhere inside the
 * truncation band), margin (int32_t)ceilf(trunc_margin / voxel_size) -- 5 for the reference's grid: a surface closer to a face
 * than this has part of its band clipped by the grid.  Host arithmetic only: needs no device.
 */
typedef struct tsdf_extent_params { float weight_thresh; float band; int32_t margin; } tsdf_extent_params;
typedef struct tsdf_extent {
    uint64_t n_observed, n_surface;
    uint64_t sum[3];      /* over surface voxels: x, y, z                       */
    uint64_t sum2[6];     /* xx, yy, zz, xy, xz, yz                             */
    uint64_t border[6];   /* surface voxels within `margin` voxels of the faces */
                          /* x-, x+, y-, y+, z-, z+ of the GLOBAL grid          */
                          /* (x < margin; x >= dim_x - margin; and so on)       */
    int32_t lo[3], hi[3]; /* inclusive index bounds of the surface voxels;      */
                          /* lo = dims, hi = -1 when n_surface == 0             */
} tsdf_extent;
int tsdf_extent_params_default(const tsdf_config *cfg, tsdf_extent_params *out);
/*
 * The record of one handle, a plain one or a borrowed batch member or group slab.  Applies the handle's collected frames first
 * (through its batch or group where it has one), queues everything on the handle's stream and returns when *out is on the host.
 * Reads the volume only: not one bit of TSDF, weights, summary words, labels or colours changes.  Unlike raycast and merging it
 * takes a z-slab handle: indices, bounds and the z faces are then in GLOBAL z and the record covers the slab's voxels.
 * Refused with TSDF_ERR_INVALID (this call, tsdf_batch_extents and tsdf_group_extent): a NULL argument; a weight_thresh that
 * is not finite; a band that is not finite or outside (0, 1]; a negative margin; a slab of so many voxels that voxels *
 * (largest global dim)^2 reaches 2^64 (the second moments could wrap).
 */
int tsdf_volume_extent(tsdf_volume *vol, const tsdf_extent_params *p, tsdf_extent *out);
/*
 * The record of two disjoint sets of voxels of one grid from the records of each: sums added, lo by min, hi by max.  The
 * extent of a whole grid equals the combination of its slabs' extents.  out may be a or b.  Host arithmetic only.
 */
int tsdf_extent_combine(const tsdf_extent *a, const tsdf_extent *b, tsdf_extent *out);
/*
 * Metric form of a record, in double: voxel index i sits at origin + i * voxel_size in the base frame.  centroid_base = origin +
 * (sum / n) * voxel_size; centroid_world = base2world applied to it; cov_base = (sum2 / n - mean * mean^T) * voxel_size^2 in the
 * order xx, yy, zz, xy, xz, yz; lo_base / hi_base = the outer corners of the bounding voxels, origin + (lo - 0.5) * voxel_size
 * and origin + (hi + 0.5) * voxel_size (a voxel is the cube around its centre).  Refuses n_surface == 0.  Host arithmetic only.
 * (The struct has a tag and no typedef: C keeps tags apart from function names, so both can be called tsdf_extent_metric.)
 */
struct tsdf_extent_metric {
    double centroid_base[3], centroid_world[3];
    double cov_base[6];
    double lo_base[3], hi_base[3];
};
int tsdf_extent_metric(const tsdf_config *cfg, const tsdf_extent *e, struct tsdf_extent_metric *out);
/*
 * The grid to move an object into (tsdf_create, then tsdf_fuse_volume): *out_cfg starts as a copy of *cfg; per axis
 * origin[i] = cfg->origin[i] + (float)(e->lo[i] - pad_voxels) * voxel_size -- two rounded float32 operations; the index may be
 * negative: the grid grows outward -- and dim[i] = hi[i] - lo[i] + 1 + 2 * pad_voxels rounded up to a multiple of dim_multiple
 * (batches need 4); z_begin = 0, z_end = dim_z.  Refuses n_surface == 0, pad_voxels < 0, dim_multiple < 1 and a result
 * tsdf_create would refuse.  Host arithmetic only; whether and when to re-grid stays the caller's decision.
 */
int tsdf_extent_regrid(const tsdf_config *cfg, const tsdf_extent *e, int32_t pad_voxels, int32_t dim_multiple,
                       tsdf_config *out_cfg);

/*
 * Grid origin of a new object volume from its first (masked) depth frame, on the device: the per-axis
 * minimum over pixels with depth > 0 of the back-projected point, starting from 1000 -- what
 * Object::Object computes on the host before it constructs its TSDF (ref: src/Object.cpp:37-49, with the
 * instance mask of ref: src/Engine.cpp:192-193; mask_dev may be NULL).  Bit-identical to that loop for every
 * frame without NaN samples (a minimum is order-independent); with NaN samples the reference's running std::min
 * depends on the raster order (a NaN replaces the minimum, the next valid pixel replaces the NaN) whereas this
 * reduction ignores them.  The call waits for all work queued on the device (whatever stream produced depth_dev,
 * e.g. tsdf_convert_depth_u16 on a handle's stream) before it reads the frame, and returns when the result is on
 * the host.
 */
int tsdf_object_origin(int32_t device, const float *depth_dev, const uint8_t *mask_dev, int32_t im_height,
                       int32_t im_width, const float cam_K[9], float origin_out[3]);

/*
 * Batched per-object fusion: the reference keeps one small TSDF per object instance and feeds
 * each of them depth * (its instance mask) for every keyframe (ref: src/Engine.cpp:172-233,
 * src/Object.cpp:67,143-166).  A batch owns n volumes (own grid, origin and base pose each; same
 * device and image size; dim_x % 4 == 0) and integrates one frame into ALL of them per call.
 * masks_dev: n device pointers to im_height*im_width {0,255} bytes (entry or whole array may be
 * NULL = unmasked).  Volumes are borrowed with tsdf_batch_volume() for download / save /
 * extraction; they are destroyed with the batch.
 * How the frames reach the volumes is the library's choice, the result is the same bits: either one
 * kernel launch over all members per call, or -- deferral, the default for batches of few or large
 * members, as for a single handle (tsdf_set_deferral on the FIRST member sets the frames per flush, 0 / 1
 * switches it off) -- the frame is copied into the batch's pool in HBM (the depth image once, the masks
 * by one gather launch; the caller's buffers are free again under the batch stream's order) and every
 * 32 collected frames are applied by one fused launch per member.  tsdf_batch_sync and every call that
 * observes or integrates into a member through its borrowed handle apply the collected frames first.
 */
typedef struct tsdf_batch tsdf_batch;
int tsdf_batch_create(const tsdf_config *cfgs, int32_t n, tsdf_batch **out);
int tsdf_batch_destroy(tsdf_batch *batch);
int tsdf_batch_size(const tsdf_batch *batch);
int tsdf_batch_volume(tsdf_batch *batch, int32_t i, tsdf_volume **vol);
int tsdf_batch_integrate_device(tsdf_batch *batch, const float *depth_dev, const uint8_t *const *masks_dev,
                                const float cam2world[16]);
int tsdf_batch_sync(tsdf_batch *batch);
/*
 * Every member of the batch rendered into one image (tsdf_raycast rule per member, with that member's own cam2base, voxel
 * size and truncation): per pixel the nearest hit wins, ties go to the lower member index; member_dev = that index or -1.
 * depth / normal are the winning member's own bits.  Device outputs, each may be NULL but not all; queued on the batch's
 * stream after its collected frames.
 */
int tsdf_batch_raycast_device(tsdf_batch *batch, const tsdf_raycast_params *p, const float cam2world[16], float *depth_dev,
                              float *normal_dev, int32_t *member_dev);

/*
 * Joint tracking against a batch: the camera pose from all the objects a caller trusts, by one call, and each object's own
 * system at that pose (an object whose system no longer agrees with the camera's motion was moved or associated wrongly: its
 * sqrt(S[27] / S[28]) stands out, and the caller can leave it out of the next call or solve its system for the object's own
 * motion).  tsdf_track's rule with three changes, stated in csrc/tsdf_batch_track.hip.h and restated in
 * tests/batch_track_spec.py: the poses are taken in the reference camera's frame (the members have base frames of their own:
 * no base2world enters), the model is tsdf_batch_raycast_device's render at the guess (depth, normal, member), and a pair
 * belongs to the member of its model pixel.  The joint system of an iteration sums the pairs of the members with
 * member_use[m] != 0 (host, tsdf_batch_size bytes; NULL = all); the solve, the lost test, the levels and every field of
 * `out` are tsdf_track's on that system.  member_systems (host, tsdf_batch_size x 29 doubles in tsdf_track_system's layout, or
 * NULL: the pass is not run): one more association pass after the last iteration, at the final estimate and at the finest
 * level that has iters > 0 (level 0 when none has), for EVERY member, used or not.  Its counts (entry 28) and sums are those
 * of a later pass than the one out->inliers and out->rmse report.  On a lost track the pose is the guess's own bits and every
 * system is all +0.0.  Two spheres alone leave the rotation about the line through their centres free: keep a box in play.
 * Applies the batch's collected frames, renders once into scratch the batch owns, queues every iteration and the member pass
 * on the batch's stream without a round trip per iteration, makes one copy and one wait; reads the volumes only.  Lost is
 * TSDF_OK with status 2.  ray.im_height / ray.im_width must be the batch's image size; a z-slab member is refused.
 */
int tsdf_batch_track(tsdf_batch *batch, const tsdf_track_params *p, const float *depth_dev, const uint8_t *mask_dev,
                     const uint8_t *member_use, const float guess_cam2world[16], tsdf_track_result *out,
                     double *member_systems);
/* One member pass: the model rendered at ref_cam2world, the pairs of level `level` taken at cam2world, for every member. */
int tsdf_batch_track_system(tsdf_batch *batch, const tsdf_track_params *p, const float *depth_dev, const uint8_t *mask_dev,
                            const float ref_cam2world[16], const float cam2world[16], int32_t level,
                            double *member_systems);
/*
 * The same pass over images the caller supplies (what tsdf_associate_count is to association): model depth, normal (x 3) and
 * member index per pixel, ray.im_height x ray.im_width; member ids outside [0, n_members) belong to no member; n_members in
 * 1..65536.  Waits for all work queued on the device before it reads; returns when the systems are on the host.
 */
int tsdf_track_member_systems(int32_t device, const tsdf_track_params *p, const float *model_depth_dev,
                              const float *model_normal_dev, const int32_t *member_dev, int32_t n_members,
                              const float *depth_dev, const uint8_t *mask_dev, const float ref_cam2world[16],
                              const float cam2world[16], int32_t level, double *member_systems);
/*
 * The extent (tsdf_volume_extent) of every member of a batch in ONE launch (members differ in dims; the batch's slice map indexes {member, slice}): out receives
 * tsdf_batch_size records.  Applies the batch's collected frames first, queues everything on the batch's stream and returns
 * when all records are on the host.  Each record equals tsdf_volume_extent on that member's borrowed handle.
 */
int tsdf_batch_extents(tsdf_batch *batch, const tsdf_extent_params *p, tsdf_extent *out /* tsdf_batch_size records */);

/*
 * Association: which object of a batch each instance mask of a live frame shows -- step 1 of the reference's per-instance
 * object loop (ref: src/Engine.cpp:172-233, TrackObjectPoints at src/Engine.cpp:356-496), on the dense models.  The batch is
 * rendered at cam2world (tsdf_batch_raycast_device: member[p] in {-1, 0..M-1}, rdepth[p]); a counting kernel compares the
 * render with the live depth under every mask (csrc/tsdf_associate.hip.h states the per-pixel rule); the host assigns.  Both
 * are restated in tests/associate_spec.py.
 *   Per pixel p of the live frame d = depth[p]:
 *     live valid   isfinite(d) && near_m < d && d <= far_m (ray.near_m / ray.far_m; tsdf_track's test)
 *     in mask k    masks[k*H*W + p] >= 128 (the masked Integrate's test); masks: K contiguous H*W byte images (MaskRCNN layout)
 *     rendered     0 <= member[p] < M
 *     class        of a rendered pixel with valid live depth, r = d - rdepth[p] (float32):  agree if fabsf(r) <= depth_tol_m,
 *                  front if r < -depth_tol_m (something occludes the model: the reference's occlusion assumption,
 *                  ref: src/Engine.cpp:399), behind otherwise (the camera sees through where the model has a surface)
 *   Counts, uint32, one block of 3*K*M + 3*K + 4*M words in this order:
 *     overlap[k][m][c]  c in {agree, front, behind}: pixels in mask k rendered as member m, of class c
 *     mask[k][j]        j in {in mask, and live valid, and live valid and not rendered} (the last: what no object explains)
 *     member[m][c]      c in {agree, front, behind, rendered with live not valid}, over the whole image
 *   Assignment, host arithmetic, exact and deterministic: a = overlap[k][m][agree], u = mask[k][1] + member[m][0] - a (the
 *   union of the mask's valid pixels and the member's agreeing ones; 64-bit).  (k, m) is a candidate iff a >= min_pixels and
 *   (double)a >= (double)min_iou * (double)u; with a label block also iff mask_label[k] == member_label[m] ||
 *   member_score[m] > 1.1f * mask_score[k] (float32; the reference's c3 || c4, ref: src/Engine.cpp:437-443).
 *   one_to_one = 1: candidates are accepted greedily by IoU a / u in descending order -- compared exactly, a1 * u2 against
 *   a2 * u1 as integers -- ties to the lower k, then the lower m; a candidate whose mask or member is taken is skipped.
 *   one_to_one = 0: each mask takes its best candidate, ties to the lower m.
 *   Outputs: assign[k] = the member or -1 (no candidate: "create an object"); iou[k] = (float)((double)a / (double)u), 0 when
 *   unassigned.  A block with some overlap[k][m][agree] above mask[k][1] or member[m][0] cannot come from an image and is
 *   refused.
 * Deviations from the reference: it takes the FIRST object in its set's order that passes (not the best), counts sparse
 * ObjectPoints projected into the keyframe (not pixels of a render) and needs each point mnDist pixels inside the mask's
 * contour (an erosion, not applied here); its contour-shape test c2 (matchShapes) is disabled there and absent here.
 *   depth_tol_m   finite, > 0                        min_pixels   >= 1
 *   min_iou       in [0, 1]                          one_to_one   0 or 1
 * tsdf_associate_params_default: ray = tsdf_raycast_params_default(cfg); depth_tol_m = cfg->trunc_margin (a fused surface sits
 * within a fraction of the truncation band of the depth that made it, so an agreeing pixel is off by less; a looser tolerance
 * would take a nearby occluder for the model); min_pixels 25 (the reference's Engine.mMinArea, ref: config/TUM3.yaml:88);
 * min_iou 0.25 (a mask half covered by a model that is twice its size still passes -- partial views and fusion holes are
 * common -- while a mask that merely touches a neighbour does not); one_to_one 1 (one instance is one object in a keyframe).
 * Host arithmetic only: needs no device.
 */
typedef struct tsdf_associate_params {
    tsdf_raycast_params ray;   /* render; near_m / far_m are also the live depth range */
    float depth_tol_m;         /* finite, > 0 */
    int32_t min_pixels;        /* >= 1 */
    float min_iou;             /* in [0, 1] */
    int32_t one_to_one;        /* 0 or 1 */
} tsdf_associate_params;
typedef struct tsdf_associate_labels {   /* optional; every pointer is a host array */
    const uint16_t *mask_label; const float *mask_score;       /* K each */
    const uint16_t *member_label; const float *member_score;   /* M each */
} tsdf_associate_labels;

int tsdf_associate_params_default(const tsdf_config *cfg, tsdf_associate_params *out);
/*
 * The counts over images the caller supplies (ray.im_height x ray.im_width each): member_dev int32, rdepth_dev and depth_dev
 * floats, masks_dev K images of bytes, all device pointers on `device`; 1 <= k <= 256, 1 <= n_members <= 65536.  Waits for
 * all work queued on the device (whatever stream produced the images) before it reads, and returns when the block is in
 * counts_host (3*k*n_members + 3*k + 4*n_members words).
 */
int tsdf_associate_count(int32_t device, const tsdf_associate_params *p, const int32_t *member_dev,
                         const float *rdepth_dev, int32_t n_members, const float *depth_dev,
                         const uint8_t *masks_dev, int32_t k, uint32_t *counts_host);
/* The assignment on a count block (labels may be NULL).  Host arithmetic only: needs no device. */
int tsdf_associate_assign(const tsdf_associate_params *p, const uint32_t *counts_host, int32_t k,
                          int32_t n_members, const tsdf_associate_labels *labels,
                          int32_t *assign_out, float *iou_out);
/*
 * The product call: applies the batch's collected frames, renders every member at cam2world into scratch the batch owns,
 * counts under the k masks (masks_dev: k contiguous im_height x im_width byte images; depth_dev: the live frame) and assigns;
 * returns when assign_out / iou_out (k each) and, unless NULL, counts_host (3*k*M + 3*k + 4*M words, M = tsdf_batch_size)
 * are on the host.  Everything is queued on the batch's stream; the volumes are only read.  Whole-grid members only.
 * Refused: a NULL argument (but counts_host and labels), k outside 1..256, ray.im_height / im_width unlike the batch's image
 * size, and every invalid parameter above.
 */
int tsdf_batch_associate(tsdf_batch *batch, const tsdf_associate_params *p, const float cam2world[16],
                         const float *depth_dev, const uint8_t *masks_dev, int32_t k,
                         const tsdf_associate_labels *labels, uint32_t *counts_host /* may be NULL */,
                         int32_t *assign_out, float *iou_out);

/*
 * Geometric segmentation of a live depth frame and the refinement of instance masks by it -- what the reference runs before
 * it touches any object: mpDoN->extract (ref: src/DoN.cpp:129-270: normals at a small and a large radius, the points where
 * they differ -- difference of normals, "DoN" -- clustered by Euclidean distance) and fuse_segments (ref:
 * src/Engine.cpp:300-338: a cluster goes to an instance only if more than mOverlap of it lies mnDist pixels inside the
 * instance's mask, and only those pixels go on into the object, :216-217).  There it is a PCL pipeline on the CPU; here the
 * rule is this project's own, stated operation by operation in csrc/tsdf_segment.hip.h and restated in
 * tests/segment_spec.py; the device's outputs equal the restatement's bit for bit.
 *   Points    p = (u, v) with d = depth[p] is valid iff isfinite(d) && near_m < d && d <= far_m (tsdf_track's test); its point
 *             ((u - cx) / fx * d, (v - cy) / fy * d, d), float32 in this order, is quantised per coordinate to the int32
 *             clamp(rintf(c * 8192.0f), -2^29, 2^29): 2^-13 m.
 *   Normal    at radius r: a lattice of 17 x 17 taps around p, tap (i, j) at pixel (u + i sx, v + j sy), sx = ceil(hx / 8) with
 *             hx = clamp(floorf(fx * r / d), 1, W) (sy, hy from fy, H); a tap counts iff inside the image, valid and within
 *             rintf(r * 8192) quanta of p's point (integer squared distance).  Integer count n, first and second moments of
 *             Q - P; the covariance S2 / n - (S1 / n)(S1 / n)^T in double; 5 cyclic Jacobi sweeps in double; the normal is the
 *             eigenvector of the smallest eigenvalue, turned toward the camera (n . P <= 0).  No normal when n < 3 or the
 *             middle eigenvalue is not above 1.0 (one squared quantum).
 *   DoN       don = 0.5 * |n_small - n_large| in double; kept iff both normals exist and don > (double)don_thresh; the image
 *             holds (float)don, 0 where a normal is missing.
 *   Clusters  kept 4-neighbours are joined iff their points lie within rintf(seg_radius_m * 8192) quanta; components of fewer
 *             than min_cluster or more than max_cluster pixels are dropped, the others numbered 1..C by their smallest flat
 *             pixel index.  The cluster image is int32, 0 = none.
 *   Refine    masks: K contiguous H*W byte images (tsdf_batch_associate's layout), in(k, p) iff the byte >= 128; deep(k, p)
 *             iff in(k, q) for every q of the (2 inset + 1)^2 square around p (outside the image: not in).  uint32 counts in
 *             one block of C + C*K words: size[c] at c - 1, inside[c][k] = #{p in cluster c: deep(k, p)} at C + (c - 1) K + k.
 *             accept(c, k) iff (float)inside / (float)size > overlap (float32, strict).  out[k][p] = 255 iff p is in a
 *             cluster c, deep(k, p) and accept(c, k); otherwise 0.  The refined masks are {0, 255} images in the layout
 *             tsdf_batch_integrate_device, tsdf_batch_associate and tsdf_track take.
 * Deviations from the reference: a subsampled lattice stands in for PCL's full radius neighbourhood; connectivity is
 * 4-neighbour in the image, not a kd-tree search; normals face the camera, not PCL's (FLT_MAX, ...) viewpoint; the erosion is
 * a square window, not the distance to the mask's polygon; the cloud has no RGB.
 *   near_m, far_m    0 <= near < far <= 32, finite       small / large / seg radius   finite, in (0, 32], small < large
 *   don_thresh       finite, > 0                         min_cluster >= 1, max_cluster >= min_cluster
 *   overlap          in (0, 1]                           inset   0..16
 * tsdf_segment_params_default: cam_K and the image size of cfg, near 0, far = cfg->max_depth, radii 0.05 / 0.5 m, don_thresh
 * 0.1, seg_radius 0.05 m (ref: config/TUM3.yaml:75-78), min_cluster 15 and max_cluster 1000000 (ref: src/DoN.cpp:47), overlap
 * 0.5 (ref: config/TUM3.yaml:90), inset 2 (mnDist = 1.0, :85: a contour runs through the mask's boundary pixels, so a
 * distance above 1 needs the two rings around a pixel in the mask).  Host arithmetic only: needs no device.
 */
typedef struct tsdf_segment_params {
    float cam_K[9];
    int32_t im_height, im_width;
    float near_m, far_m;
    float small_radius_m, large_radius_m;
    float don_thresh;
    float seg_radius_m;
    int32_t min_cluster, max_cluster;
    float overlap;
    int32_t inset;
} tsdf_segment_params;
int tsdf_segment_params_default(const tsdf_config *cfg, tsdf_segment_params *out);
/*
 * A segmenter owns the scratch of one image size on one device (about 40 bytes per pixel) and a stream; every call below
 * queues its work on that stream (tsdf_segmenter_set_stream: the caller's, NULL = its own again), only reads its inputs and
 * returns when its work is done and the host outputs are there.  Refused, with tsdf_last_error set: an invalid parameter (see
 * above; checked first), a NULL argument other than those marked, k outside 1..256, p->im_height / im_width unlike the
 * segmenter's, masks_out_dev == masks_dev, and a count block C + C*k above 2^24 words.
 */
typedef struct tsdf_segmenter tsdf_segmenter;
int tsdf_segmenter_create(int32_t device, int32_t im_height, int32_t im_width, tsdf_segmenter **out);
int tsdf_segmenter_destroy(tsdf_segmenter *seg);
int tsdf_segmenter_set_stream(tsdf_segmenter *seg, void *hip_stream);
/* depth_dev: H*W floats (metres); don_dev: H*W floats or NULL; cluster_dev: H*W int32; *n_clusters = C. */
int tsdf_segment_depth_device(tsdf_segmenter *seg, const tsdf_segment_params *p, const float *depth_dev,
                              float *don_dev /* may be NULL */, int32_t *cluster_dev, int32_t *n_clusters);
/*
 * Refines k masks by any cluster image with labels in 0..n_clusters (a value outside 1..n_clusters counts as none);
 * masks_out_dev: k*H*W bytes; counts_host: n_clusters + n_clusters*k words, or NULL.
 */
int tsdf_segment_refine_masks_device(tsdf_segmenter *seg, const tsdf_segment_params *p, const int32_t *cluster_dev,
                                     int32_t n_clusters, const uint8_t *masks_dev, int32_t k, uint8_t *masks_out_dev,
                                     uint32_t *counts_host /* may be NULL */);
/* The product call: tsdf_segment_depth_device, then the refinement of the k masks by its clusters. */
int tsdf_segment_frame(tsdf_segmenter *seg, const tsdf_segment_params *p, const float *depth_dev,
                       const uint8_t *masks_dev, int32_t k, uint8_t *masks_out_dev,
                       int32_t *cluster_dev /* may be NULL */, int32_t *n_clusters);

/*
 * Lidar scans.  The reference's second sensor (mSensor == 1) feeds its object loop an image of RANGES, distances along the
 * ray, made from a Velodyne scan (ref: examples/label_instance_lidar.cpp:76-77,126; src/Utility.cpp:40-57,374-419), and every
 * consumer that turns such a pixel into a point divides by the ray's length (ref: src/Object.cpp:613-620, src/DoN.cpp:89-96).
 * Everything else in this header takes z-depth; the calls below make z-depth out of a scan or out of a range image, on the
 * device, so that the whole of it serves the second sensor as well.  The rule is stated exactly in csrc/tsdf_scan.hip.h and
 * restated in tests/scan_spec.py; every pointer here is host memory, borrowed for the call only.
 *   points_host   n_points x 4 floats in the KITTI .bin layout (x, y, z, intensity; the intensity is ignored), in scan order:
 *                 where several points fall into one pixel the one with the highest index stays, as in the reference's loop.
 *                 0 <= n_points <= 4294967295 (2^32 - 1: a point's index + 1 is the upper word of its pixel's 64-bit key);
 *                 n_points == 0 is valid (points_host may then be NULL) and gives all-zero images
 *   velo2img      3 x 4 row-major, scanner frame to pixels times depth; finite.  A point is kept when (velo2img * point)[0]
 *                 >= 2 (ref: src/Utility.cpp:53, the reference's guard as it stands) and its pixel (u, v), truncated, has
 *                 1 <= u < width and 1 <= v < height: row 0 and column 0 are never written (ref: :405)
 *   cam_K         the camera of the range image, finite with fx, fy != 0:
 *                 depth = range / sqrtf(((u - cx) / fx)^2 + ((v - cy) / fy)^2 + 1) where 0 < range <= FLT_MAX, else 0
 * tsdf_scan_projection composes velo2img = P_rect * [R_rect 0; 0 1] * [R_velo t_velo; 0 1] (ref: src/Utility.cpp:42-49) in
 * tsdf_multiply_matrix's fp32 operation order; host arithmetic only, needs no device.  The library embeds no calibration.
 */
int tsdf_scan_projection(const float P_rect[12], const float R_rect[9], const float R_velo[9], const float t_velo[3],
                         float velo2img_out[12]);
/*
 * A tsdf_scanner projects scans into images of one size on one device; it owns the key image, the points' staging and the
 * output images (allocated at the first call that needs them).  One scanner may be driven from one thread at a time.
 *   tsdf_scan_project         the scan's range image into range_host, its z-depth image into depth_host (both im_height x
 *                             im_width floats, 0 where no point fell) and the number of written pixels into *n_pixels.  Each
 *                             of the three may be NULL, not all of them; cam_K may be NULL when depth_host is.  Returns with
 *                             the images on the host.  Successive scans through one scanner do not see each other.
 *   tsdf_scan_range_to_depth  the conversion alone, for a caller who holds a range image already; returns with depth_host
 *                             written.  range_host and depth_host may be the same buffer.
 * depth_host is what tsdf_integrate, tsdf_group_integrate and -- uploaded -- tsdf_object_origin, the batch, segmentation and
 * tracking calls take as their depth frame, unchanged.
 */
typedef struct tsdf_scanner tsdf_scanner;
int tsdf_scanner_create(int32_t device, int32_t im_height, int32_t im_width, tsdf_scanner **out);
int tsdf_scanner_destroy(tsdf_scanner *scanner);
int tsdf_scan_project(tsdf_scanner *scanner, const float velo2img[12], const float cam_K[9], const float *points_host,
                      int64_t n_points, float *range_host, float *depth_host, int64_t *n_pixels);
int tsdf_scan_range_to_depth(tsdf_scanner *scanner, const float cam_K[9], const float *range_host, float *depth_host);
/*
 * TSDF::Integrate for the second sensor: tsdf_integrate's call shape and behaviour, deferral included (the frames of these
 * calls are collected with tsdf_integrate's and applied with them, in call order), for an image of ranges or for the scan
 * itself.  The image size and cam_K are the handle's (a handle whose cam_K is not finite or has fx or fy == 0 is refused).
 *   tsdf_integrate_range   range_host: im_height x im_width floats; copied as it is and converted to z-depth on the device
 *                          on its way into the frame's slot, as tsdf_integrate_u16 converts a 16-bit frame
 *   tsdf_integrate_scan    points in, fused: projected on the device straight into the frame's slot; the image never
 *                          leaves the device.  The handle's scan memory is allocated at the first such call
 * Equal, bit for bit, to tsdf_integrate of tsdf_scan_range_to_depth's, respectively tsdf_scan_project's, depth_host.
 */
int tsdf_integrate_range(tsdf_volume *vol, const float *range_host, const float cam2world[16]);
int tsdf_integrate_scan(tsdf_volume *vol, const float velo2img[12], const float *points_host, int64_t n_points,
                        const float cam2world[16]);
/*
 * Filling the gaps between beams.  A 64-beam scan writes a few pixels in a hundred, in rows one beam apart; Integrate samples
 * the nearest pixel and skips a voxel whose pixel is empty, so the sparse image fuses isolated rows of voxels.  The fill
 * interpolates INVERSE depth between the nearest sources on either side of an empty pixel, along rows first (u pass) and
 * then along columns (v pass, which also takes u-filled pixels as sources); it never extrapolates and never bridges a
 * relative depth difference above jump_rel.  Off unless asked for: nothing above changes.  The rule is stated exactly in
 * csrc/tsdf_scan_fill.hip.h and restated in tests/scan_fill_spec.py.
 *   max_span_u, max_span_v   0 ... 16: the largest distance in pixels between two sources that the pass bridges; 0 or 1
 *                            turns the pass off
 *   jump_rel                 finite, >= 0: a pair a, b is bridged only if |a - b| <= jump_rel * min(a, b)
 * tsdf_scan_fill_params_default gives 5, 8, 0.05f: the gap widths of a 64-beam revolution in a 1242 x 375 image (one beam
 * spacing is closed, two are not) and a conservative jump; choices, not measurements.  Host only, needs no device.
 *   tsdf_scan_fill_depth         any sparse z-depth image of the scanner's size in; the filled image into filled_host, the
 *                                kind image (0 empty, 1 measured, 2 filled by the u pass, 3 by the v pass) into kind_host,
 *                                the number of filled pixels into *n_filled.  Each of the three may be NULL, not all of
 *                                them.  filled_host may be depth_host.  An unfilled pixel keeps its input bits
 *   tsdf_scan_project_filled     tsdf_scan_project's depth image through tsdf_scan_fill_depth, without the image visiting
 *                                the host in between; the same three outputs
 *   tsdf_integrate_range_filled, tsdf_integrate_scan_filled
 *                                tsdf_integrate_range and tsdf_integrate_scan, deferral included, with the fill between
 *                                the z-depth image and the frame's slot.  Equal, bit for bit, to tsdf_integrate of the
 *                                image tsdf_scan_fill_depth, respectively tsdf_scan_project_filled, returns
 */
typedef struct tsdf_scan_fill_params {
    int32_t max_span_u, max_span_v;
    float jump_rel;
} tsdf_scan_fill_params;
int tsdf_scan_fill_params_default(tsdf_scan_fill_params *out);
int tsdf_scan_fill_depth(tsdf_scanner *scanner, const tsdf_scan_fill_params *params, const float *depth_host,
                         float *filled_host, uint8_t *kind_host, int64_t *n_filled);
int tsdf_scan_project_filled(tsdf_scanner *scanner, const float velo2img[12], const float cam_K[9],
                             const tsdf_scan_fill_params *params, const float *points_host, int64_t n_points,
                             float *depth_host, uint8_t *kind_host, int64_t *n_filled);
int tsdf_integrate_range_filled(tsdf_volume *vol, const tsdf_scan_fill_params *params, const float *range_host,
                                const float cam2world[16]);
int tsdf_integrate_scan_filled(tsdf_volume *vol, const float velo2img[12], const tsdf_scan_fill_params *params,
                               const float *points_host, int64_t n_points, const float cam2world[16]);
/*
 * Marking the ground of a scan.  The reference's lidar front end sorts a scan into a spherical image of n_rings x n_columns
 * cells (ref: src/Utility.cpp:452-496, projectPointCloud) and calls a cell ground when the step to the cell one ring above
 * it is nearly level (ref: :498-553, groundRemoval); both run on the CPU and are dormant at its call site
 * (ref: examples/label_instance_lidar.cpp:85-91).  Here both run on the device in front of the camera splat, so that a scan
 * can be projected or fused WITHOUT its ground returns, or with nothing else.  Off unless asked for: nothing above changes.
 * The rule uses no transcendental function on the device (the angles become tables of tangents, cosines and sines, built on
 * the host) and is stated exactly in csrc/tsdf_scan_ground.hip.h and restated in tests/scan_ground_spec.py.
 *   n_rings, n_columns      2 ... 128 and 4 ... 16384: the spherical image.  Ring r holds elevations from r * ang_res_y -
 *                           ang_bottom (inclusive) up to the next ring's; column c holds azimuths atan2(y, x) from
 *                           (c - n_columns / 2 - 0.5) * 360 / n_columns degrees (inclusive, integer n_columns / 2) up to the
 *                           next column's, x forward and y left, wrapping around
 *   ang_res_y, ang_bottom   degrees; ang_res_y > 0, every ring boundary strictly inside (-90, 90)
 *   mount_deg, tol_deg      a pair of cells is level when the step from the lower cell's point to the upper one's rises by
 *                           mount_deg +- tol_deg; tol_deg >= 0, |mount_deg| + tol_deg < 90
 *   min_range               >= 0: a point nearer than this has no cell
 *   ground_rings            0 ... n_rings - 1: the rings whose step to the ring above is looked at (0 marks nothing)
 *   mark_upper              0 or 1: whether a level step also marks its upper cell (ref: :531, commented out there).  The
 *                           cell's own step comes first, as in the reference's ascending loop: a cell below ground_rings
 *                           whose upper neighbour is empty is -1 even when the step below it is level; a cell at or above
 *                           ground_rings has no step of its own and is 1 exactly when the step below it is looked at and level
 * Every value must be finite.  tsdf_scan_ground_params_default gives the reference's literals (ref: include/Utility.hpp:52-58,
 * src/Utility.cpp:484,529): 64, 4500, 26.9 / 63, 15.1, 0, 2.5, 0.1, 63, 0.  Those cover -15.1 ... +11.8 degrees, NOT the
 * HDL-64E's +2 ... -24.8; for that sensor, with each beam at its ring's centre: ang_res_y = 26.8 / 63, ang_bottom = 24.8 +
 * ang_res_y / 2.  Host only, needs no device.
 * Where several points share a cell the one with the highest index is the cell's point, as for the camera image.  A point's
 * flag is 2 when it has no cell (not finite, on the z axis, nearer than min_range, above or below the rings), 1 when its
 * cell is ground -- every point of the cell, not only the cell's own --, else 0.
 *   tsdf_scan_mark_ground        flags_host: n_points bytes; state_host: n_rings x n_columns int8 (1 ground, 0 not, -1 the
 *                                cell or the one above it is empty); winner_host: n_rings x n_columns int32, the index of
 *                                the cell's point or -1; counts = {points with a cell, occupied cells, ground cells, ground
 *                                points}.  Each of the four may be NULL, not all of them
 *   tsdf_scan_project_ground     tsdf_scan_project of the points that select keeps (TSDF_SCAN_DROP_GROUND: flag != 1,
 *                                TSDF_SCAN_ONLY_GROUND: flag == 1), in their order: range_host and *n_pixels as
 *                                tsdf_scan_project gives them; fill_params NULL: depth_host likewise (kind_host and
 *                                n_filled must be NULL); otherwise depth_host, kind_host and *n_filled as
 *                                tsdf_scan_project_filled gives them.  *n_selected: the points kept, in the image or
 *                                not.  Every output may be NULL, not all of them
 *   tsdf_integrate_scan_ground   tsdf_integrate_scan (fill_params NULL) or tsdf_integrate_scan_filled of the points that
 *                                select keeps, deferral included.  Equal, bit for bit, to tsdf_integrate of
 *                                tsdf_scan_project_ground's depth_host
 */
typedef struct tsdf_scan_ground_params {
    int32_t n_rings, n_columns;
    float ang_res_y, ang_bottom;
    float mount_deg, tol_deg;
    float min_range;
    int32_t ground_rings;
    int32_t mark_upper;
} tsdf_scan_ground_params;
#define TSDF_SCAN_DROP_GROUND 0
#define TSDF_SCAN_ONLY_GROUND 1
int tsdf_scan_ground_params_default(tsdf_scan_ground_params *out);
int tsdf_scan_mark_ground(tsdf_scanner *scanner, const tsdf_scan_ground_params *params, const float *points_host,
                          int64_t n_points, uint8_t *flags_host, int8_t *state_host, int32_t *winner_host,
                          int64_t counts[4]);
int tsdf_scan_project_ground(tsdf_scanner *scanner, const float velo2img[12], const float cam_K[9],
                             const tsdf_scan_ground_params *ground_params, int32_t select,
                             const tsdf_scan_fill_params *fill_params, const float *points_host, int64_t n_points,
                             float *range_host, float *depth_host, uint8_t *kind_host, int64_t *n_pixels,
                             int64_t *n_filled, int64_t *n_selected);
int tsdf_integrate_scan_ground(tsdf_volume *vol, const float velo2img[12], const tsdf_scan_ground_params *ground_params,
                               int32_t select, const tsdf_scan_fill_params *fill_params, const float *points_host,
                               int64_t n_points, const float cam2world[16]);
/*
 * Tracking a scan against the fused volume, point to signed distance.  Every tsdf_integrate_scan* call needs the pose of the
 * scan; the reference takes it from a stereo SLAM run beside it (ref: examples/label_instance_lidar.cpp:36-40).  These calls
 * estimate it from the scan and the volume alone: every point, taken through the pose estimate, should land where the
 * signed distance is zero, so the trilinearly sampled TSDF value is the residual and its gradient the normal.  No image is
 * made and no camera enters it: the whole revolution takes part.  The rule is stated exactly in csrc/tsdf_scan_track.hip.h
 * and restated in tests/scan_track_spec.py; every pointer here is host memory, borrowed for the call only.  The volume is
 * only read.  Whole-grid handles only: a z-slab and a slab of a tsdf_group are refused, as tsdf_track refuses them.
 *   weight_thresh            finite: all eight corners of a point's cell must have a weight above it
 *   resid_thresh             metres, finite, > 0: a pair whose |signed distance| exceeds it is left out
 *   min_range_m, max_range_m finite, 0 <= min <= max: a point takes part when its distance from the scanner lies in
 *                            [min, max] (compared as float32 squares)
 *   n_levels, iters          1 ... 3 levels, level l takes every 2^l-th point, in scan order; iters[l] >= 0 iterations of
 *                            level l, coarsest level first (0 skips a level)
 *   min_pairs                >= 0: an iteration with fewer pairs loses the track
 *   drop_flag                -1: flags_host is not looked at; 0 ... 255: a point whose flag equals it is left out.
 *                            flags_host: n_points bytes or NULL; tsdf_scan_mark_ground's flags_host fits as it is, and
 *                            drop_flag = 1 then tracks without the ground
 *   eps_rot, eps_trans       finite, > 0: a level ends when a step turns by less than eps_rot radians and moves by less than
 *                            eps_trans metres
 * tsdf_scan_track_params_default gives 0.9, the handle's truncation distance, 2.5 (the ground rule's nearest range of a
 * ground step) and 80, 3 levels of {10, 5, 4} iterations, 300, -1, 1e-5 and 1e-5: choices, not measurements.  Host only,
 * needs no device.
 * tsdf_scan_pose composes velo2cam = [R_rect 0; 0 1] * [R_velo t_velo; 0 1] (tsdf_scan_projection's product without P_rect)
 * in tsdf_multiply_matrix's fp32 operation order; host arithmetic only, needs no device.  The caller forms velo2world =
 * cam2world * velo2cam for the guess and gets back to a camera pose with tsdf_invert_matrix and tsdf_multiply_matrix.
 *   points_host, n_points    as for tsdf_scan_project; 0 <= n_points <= 2147483584 (2^31 - 64: one lane per point).
 *                            n_points == 0 is valid (points_host may then be NULL) and loses the track
 *   guess_velo2world         4 x 4 row-major, scanner frame to world; only the first three rows are read, and they must be
 *                            finite.  Rigidity is the caller's duty
 *   tsdf_scan_track          the frames the handle has collected are applied first; returns when the result is on the host.
 *                            status 0: the finest level that ran ended by the eps test, 1: its iterations ran out, 2: lost
 *                            -- not an error: TSDF_OK, and velo2world is then the guess's own bits.  iters_run per level;
 *                            pairs and rmse (metres) of the last iteration that ran
 *   tsdf_scan_track_system   the 29 sums of ONE pass of `level` (0 <= level < n_levels) at the pose velo2world, no step:
 *                            21 of J^T J (upper triangle, row-major), 6 of J^T r, sum r^2, the pair count; returns when
 *                            they are on the host.  What the tests hold against the restatement
 * Two calls with the same volume, scan and pose give the same bits: the sums are made in a fixed order.
 */
typedef struct tsdf_scan_track_params {
    float weight_thresh, resid_thresh;
    float min_range_m, max_range_m;
    int32_t n_levels; int32_t iters[3];
    int32_t min_pairs;
    int32_t drop_flag;
    float eps_rot, eps_trans;
} tsdf_scan_track_params;
typedef struct tsdf_scan_track_result { float velo2world[16]; int32_t status; int32_t iters_run[3]; int32_t pairs; float rmse; } tsdf_scan_track_result;
int tsdf_scan_track_params_default(const tsdf_config *cfg, tsdf_scan_track_params *out);
int tsdf_scan_pose(const float R_rect[9], const float R_velo[9], const float t_velo[3], float velo2cam_out[16]);
int tsdf_scan_track(tsdf_volume *vol, const tsdf_scan_track_params *p, const float *points_host, int64_t n_points,
                    const uint8_t *flags_host /* may be NULL */, const float guess_velo2world[16], tsdf_scan_track_result *out);
int tsdf_scan_track_system(tsdf_volume *vol, const tsdf_scan_track_params *p, const float *points_host, int64_t n_points,
                           const uint8_t *flags_host, const float velo2world[16], int32_t level, double system_out[29]);

/*
 * One grid over several devices in ONE process.  The reference's host is a C++ program that owns its TSDFs directly
 * (ref: include/tsdf.hpp:22-43; src/Engine.cpp:170-172 drives distinct TSDFs from one loop), so a C++ caller must be
 * able to span the node without a process per GPU.  tsdf_group_create cuts the grid of *cfg (its z_begin / z_end /
 * device fields are ignored) into n_slabs contiguous z-slabs -- slab i holds z in [i*dim_z/n, (i+1)*dim_z/n) and lives
 * on devices[i], with its own stream; ordinals may repeat (several slabs on one device).  Needs n_slabs <= dim_z.
 *   tsdf_group_integrate         TSDF::Integrate for the whole grid (ref: src/tsdf.cu:135-168): the caller's frame is
 *                                copied once into pinned memory; deferred like tsdf_integrate -- 32 collected frames go
 *                                out as one copy and one fused launch per slab (tsdf_group_set_deferral(g, 0): one
 *                                asynchronous copy per slab and its kernel per call); no synchronisation between
 *                                devices and no collective (voxels are independent); returns without waiting
 *   tsdf_group_integrate_frames  a known sequence from host frames: per pass of up to 32 frames, one copy of the
 *                                frames to every device and one fused launch per slab (tsdf_integrate_frames_device)
 *   tsdf_group_download          the whole grid in z order (== one handle's tsdf_download, bit for bit)
 *   tsdf_group_extract_*         lists of the whole grid in grid order; zero crossings and the mesh fetch slice z_end
 *                                from the next slab device to device (hipMemcpyPeerAsync, dim_y*dim_x*8 bytes per
 *                                boundary); one host thread per slab, so the devices extract concurrently
 *   tsdf_group_save_*            the reference's files (ref: src/tsdf.cu:107-132,170-218), byte-identical to a
 *                                whole-grid handle's
 *   tsdf_group_volume            borrow slab i's handle (tsdf_device_ptrs, tsdf_copy_slices, ...); it is
 *                                destroyed with the group
 */
typedef struct tsdf_group tsdf_group;
int tsdf_group_create(const tsdf_config *cfg, const int32_t *devices, int32_t n_slabs, tsdf_group **out);
int tsdf_group_destroy(tsdf_group *group);
int tsdf_group_size(const tsdf_group *group);
int64_t tsdf_group_voxels(const tsdf_group *group);
int tsdf_group_volume(tsdf_group *group, int32_t i, tsdf_volume **vol);
int tsdf_group_integrate(tsdf_group *group, const float *depth_host, const float cam2world[16]);
int tsdf_group_integrate_frames(tsdf_group *group, const float *const *depth_host, const float *cam2world,
                                int32_t n_frames);
/* Frames tsdf_group_integrate collects per pass (deferred integration as for tsdf_integrate; default 32, 0 = none). */
int tsdf_group_set_deferral(tsdf_group *group, int32_t n_frames);
int tsdf_group_sync(tsdf_group *group);
int tsdf_group_reset(tsdf_group *group);
int tsdf_group_download(tsdf_group *group, float *tsdf_host, float *weight_host);
int tsdf_group_extract_surface(tsdf_group *group, float weight_thresh, float *xyz_host, int64_t capacity,
                               int64_t *count);
int tsdf_group_extract_crossings(tsdf_group *group, float weight_thresh, float *xyz_host, int64_t capacity,
                                 int64_t *count);
int tsdf_group_extract_mesh(tsdf_group *group, float weight_thresh, float *triangles_host, int64_t capacity,
                            int64_t *count);
int tsdf_group_save_ply(tsdf_group *group, const char *path, float weight_thresh);
int tsdf_group_save_mesh_ply(tsdf_group *group, const char *path, float weight_thresh);
int tsdf_group_save_bin(tsdf_group *group, const char *path);
/*
 * The extent (tsdf_volume_extent) of the whole grid: the per-slab call on every slab's device, one host thread per slab, then
 * tsdf_extent_combine.  Equal to the record of a whole-grid handle holding the same values.
 */
int tsdf_group_extent(tsdf_group *group, const tsdf_extent_params *p, tsdf_extent *out);

/* Message describing the last failure on this thread ("" when none). */
const char *tsdf_last_error(void);

/* Library version string and the offload architecture it was built for ("gfx950"). */
const char *tsdf_version(void);

/* Host-side 4x4 helpers in the reference's exact fp32 operation order
 * (ref: src/tsdf.cu:253-273 and :276-403); exported so bindings can reuse them. */
void tsdf_multiply_matrix(const float a[16], const float b[16], float out[16]);
int tsdf_invert_matrix(const float m[16], float inv_out[16]); /* 1 = ok, 0 = singular */

#ifdef __cplusplus
}
#endif
#endif /* TSDF_HIP_H */
