"""The ordering promises of include/tsdf_hip.h as a list (test infrastructure, no GPU): every entry point that takes a device
pointer, or whose comment speaks of a stream or of waiting, with the stream whose order its promise is about -- or a reason why
it makes none a caller could see broken.  tests/test_stream_cases.py holds the list to the header; DESIGN.md, section 1,
"Streams and events", says how the host code keeps the promises."""

# The stream a promise is about:
#   handle   the handle's current stream: its own, or the caller's after tsdf_set_stream (tsdf_get_stream answers it)
#   batch    the batch's stream, which the members' borrowed handles share
#   slab     each slab's own stream of a group
#   caller   the stream given to tsdf_segmenter_set_stream
#   both     the source's and the destination's stream of a merge
#   device   none: the call waits for all work queued on the device before it reads
ORDERED = {
    "tsdf_integrate": "handle",
    "tsdf_integrate_u16": "handle",
    "tsdf_integrate_rgbd": "handle",
    "tsdf_integrate_device": "handle",
    "tsdf_integrate_cam2base": "handle",
    "tsdf_integrate_masked_device": "handle",
    "tsdf_integrate_frames_device": "handle",
    "tsdf_integrate_labels_device": "handle",
    "tsdf_integrate_frames_labels_device": "handle",
    "tsdf_integrate_colour_device": "handle",
    "tsdf_convert_depth_u16": "handle",
    "tsdf_copy_slices": "handle",
    "tsdf_reset": "handle",
    "tsdf_refresh_summary": "handle",
    "tsdf_compose_labels": "handle",
    "tsdf_raycast_device": "handle",
    "tsdf_track": "handle",
    "tsdf_track_system": "handle",
    "tsdf_set_stream": "handle",
    "tsdf_get_stream": "handle",
    "tsdf_fuse_volume": "both",
    "tsdf_batch_integrate_device": "batch",
    "tsdf_batch_raycast_device": "batch",
    "tsdf_batch_track": "batch",
    "tsdf_batch_track_system": "batch",
    "tsdf_batch_extents": "batch",
    "tsdf_batch_associate": "batch",
    "tsdf_group_integrate": "slab",
    "tsdf_segmenter_set_stream": "caller",
    "tsdf_segment_depth_device": "caller",
    "tsdf_segment_refine_masks_device": "caller",
    "tsdf_segment_frame": "caller",
    "tsdf_object_origin": "device",
    "tsdf_associate_count": "device",
    "tsdf_track_member_systems": "device",
}
STREAMS = {"handle", "batch", "slab", "caller", "both", "device"}

# Entry points that take a device pointer, or stand under a comment that speaks of a stream or of waiting, and are not above.
EXEMPT = {
    "tsdf_sync": "the wait itself, for the handle's stream",
    "tsdf_batch_sync": "the wait itself, for the batch's stream",
    "tsdf_group_sync": "the wait itself, for every slab's stream",
    "tsdf_download": "synchronous by contract, host pointers only",
    "tsdf_upload": "synchronous by contract, host pointers only",
    "tsdf_count_surface": "synchronous, host outputs only",
    "tsdf_extract_surface": "synchronous, host outputs only",
    "tsdf_extract_crossings": "synchronous; its halo is read after a wait for the handle's stream, and a device halo comes from "
                              "tsdf_copy_slices, which is listed",
    "tsdf_extract_mesh": "as tsdf_extract_crossings",
    "tsdf_device_ptrs": "returns addresses and queues nothing; what is written through them is tsdf_refresh_summary's promise",
    "tsdf_raycast": "the host form of tsdf_raycast_device: returns when the images are there",
    "tsdf_volume_extent": "returns when the record is on the host, host output only",
    "tsdf_group_extent": "tsdf_volume_extent per slab on a thread each; synchronous",
    "tsdf_group_integrate_frames": "host frames through the pinned pool, one pass at a time with a host wait per pass",
    "tsdf_group_reset": "tsdf_reset per slab, which is listed",
    "tsdf_group_download": "synchronous, host pointers only",
    "tsdf_group_extract_surface": "synchronous, host outputs only",
    "tsdf_group_extract_crossings": "synchronous; the halo moves between slabs after a wait for the neighbour's stream",
    "tsdf_group_extract_mesh": "as tsdf_group_extract_crossings",
    "tsdf_destroy": "waits for every stream of the handle before it frees; nothing to observe afterwards",
    "tsdf_create": "speaks of no stream: the fill is queued on the new handle's stream, in front of everything else",
    # declarations that only stand under the comment of a neighbour that is listed
    "tsdf_batch_create": "under tsdf_batch_integrate_device's comment; waits for the members' fills before it returns",
    "tsdf_batch_destroy": "under tsdf_batch_integrate_device's comment; waits for every stream of the batch before it frees",
    "tsdf_batch_size": "under tsdf_batch_integrate_device's comment; host arithmetic only",
    "tsdf_batch_volume": "under tsdf_batch_integrate_device's comment; returns a handle and queues nothing",
    "tsdf_colour_enable": "under tsdf_integrate_rgbd's comment; allocates and clears on the handle's stream before any colour pass",
    "tsdf_download_colour": "under tsdf_integrate_rgbd's comment; synchronous, host pointer only",
    "tsdf_fuse_params_default": "under tsdf_fuse_volume's comment; host arithmetic only",
    "tsdf_group_create": "under tsdf_group_integrate's comment; queues nothing a caller can observe",
    "tsdf_group_destroy": "under tsdf_group_integrate's comment; waits for every slab's stream before it frees",
    "tsdf_group_size": "under tsdf_group_integrate's comment; host arithmetic only",
    "tsdf_group_volume": "under tsdf_group_integrate's comment; returns a handle and queues nothing",
    "tsdf_group_voxels": "under tsdf_group_integrate's comment; host arithmetic only",
    "tsdf_segmenter_create": "under tsdf_segmenter_set_stream's comment; allocates only",
    "tsdf_segmenter_destroy": "under tsdf_segmenter_set_stream's comment; waits for the segmenter's stream before it frees",
}
