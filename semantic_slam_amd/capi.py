"""ctypes binding of the C ABI in include/tsdf_hip.h and include/tsdf_hip_diag.h (libtsdf_hip.so).

This is plumbing for tests and bench.py: the same entry points a C++ caller reaches through
include/tsdf.hpp.  There is no fallback of any kind here: if the shared library is missing
or a call fails, a TsdfError is raised.
"""
import ctypes as C
import os

import numpy as np

_PKG = os.path.dirname(os.path.abspath(__file__))
# TSDF_HIP_LIB overrides the library path (A/B timing of two builds on one GPU box; tools/sweep.py)
LIB_PATH = os.environ.get("TSDF_HIP_LIB") or os.path.join(_PKG, "libtsdf_hip.so")

# every symbol the library exports: what include/tsdf_hip.h (the drop-in contract) and include/tsdf_hip_diag.h (measurement
# and tuning aids) declare together; DIAG_SYMBOLS is the second header's part (tests check both headers against these
# lists and the .so against the headers)
ABI_SYMBOLS = [
    "tsdf_config_default", "tsdf_create", "tsdf_destroy", "tsdf_reset", "tsdf_integrate",
    "tsdf_integrate_u16", "tsdf_convert_depth_u16", "tsdf_set_deferral",
    "tsdf_integrate_device", "tsdf_integrate_cam2base", "tsdf_integrate_masked_device",
    "tsdf_integrate_frames_device",
    "tsdf_sync", "tsdf_download", "tsdf_copy_slices", "tsdf_upload", "tsdf_refresh_summary", "tsdf_device_ptrs", "tsdf_slab_voxels", "tsdf_frames_per_launch", "tsdf_shortcut_stats", "tsdf_brick_list_stats", "tsdf_classification_info", "tsdf_store_stats", "tsdf_summary_stats", "tsdf_summary_words",
    "tsdf_get_config", "tsdf_last_cam2base", "tsdf_set_stream", "tsdf_get_stream",
    "tsdf_count_surface", "tsdf_extract_surface", "tsdf_extract_crossings", "tsdf_extract_mesh", "tsdf_save_mesh_ply", "tsdf_save_mesh_welded_ply", "tsdf_save_ply", "tsdf_save_bin", "tsdf_load_bin", "tsdf_save_state", "tsdf_load_state",
    "tsdf_integrate_sequence_timed", "tsdf_integrate_frames_timed", "tsdf_probe_graph_replay", "tsdf_probe_stream", "tsdf_selftest_fastdiv", "tsdf_selftest_fastdiv_band", "tsdf_selftest_round", "tsdf_selftest_tile_tables", "tsdf_set_kernel_variant", "tsdf_set_brick_shape", "tsdf_brick_shape", "tsdf_default_brick_shape", "tsdf_last_error",
    "tsdf_version", "tsdf_multiply_matrix", "tsdf_invert_matrix",
    "tsdf_labels_enable", "tsdf_compose_labels", "tsdf_integrate_labels_device", "tsdf_integrate_frames_labels_device",
    "tsdf_download_labels",
    "tsdf_colour_enable", "tsdf_integrate_colour_device", "tsdf_integrate_rgbd", "tsdf_download_colour",
    "tsdf_raycast_params_default", "tsdf_raycast_device", "tsdf_raycast", "tsdf_batch_raycast_device",
    "tsdf_track_params_default", "tsdf_track", "tsdf_track_system",
    "tsdf_photo_params_default", "tsdf_track_rgbd", "tsdf_track_rgbd_system", "tsdf_render_intensity",
    "tsdf_batch_track", "tsdf_batch_track_system", "tsdf_track_member_systems",
    "tsdf_fuse_params_default", "tsdf_fuse_volume",
    "tsdf_align_params_default", "tsdf_fuse_pose_default", "tsdf_align_volume", "tsdf_align_system", "tsdf_fuse_volume_at",
    "tsdf_fuse_volume_carry", "tsdf_upload_labels", "tsdf_upload_colour",
    "tsdf_extent_params_default", "tsdf_volume_extent", "tsdf_batch_extents", "tsdf_group_extent", "tsdf_extent_combine",
    "tsdf_extent_metric", "tsdf_extent_regrid",
    "tsdf_associate_params_default", "tsdf_associate_count", "tsdf_associate_assign", "tsdf_batch_associate",
    "tsdf_segment_params_default", "tsdf_segmenter_create", "tsdf_segmenter_destroy", "tsdf_segmenter_set_stream",
    "tsdf_segment_depth_device", "tsdf_segment_refine_masks_device", "tsdf_segment_frame",
    "tsdf_scan_projection", "tsdf_scanner_create", "tsdf_scanner_destroy", "tsdf_scan_project", "tsdf_scan_range_to_depth",
    "tsdf_integrate_range", "tsdf_integrate_scan",
    "tsdf_scan_fill_params_default", "tsdf_scan_fill_depth", "tsdf_scan_project_filled", "tsdf_integrate_range_filled",
    "tsdf_integrate_scan_filled",
    "tsdf_scan_ground_params_default", "tsdf_scan_mark_ground", "tsdf_scan_project_ground", "tsdf_integrate_scan_ground",
    "tsdf_scan_ground_tables",
    "tsdf_scan_track_params_default", "tsdf_scan_pose", "tsdf_scan_track", "tsdf_scan_track_system",
    "tsdf_object_origin", "tsdf_batch_create", "tsdf_batch_destroy", "tsdf_batch_size", "tsdf_batch_volume",
    "tsdf_batch_integrate_device", "tsdf_batch_sync",
    "tsdf_group_create", "tsdf_group_destroy", "tsdf_group_size", "tsdf_group_voxels", "tsdf_group_volume",
    "tsdf_group_integrate", "tsdf_group_integrate_frames", "tsdf_group_set_deferral", "tsdf_group_sync", "tsdf_group_reset", "tsdf_group_download",
    "tsdf_group_extract_surface", "tsdf_group_extract_crossings", "tsdf_group_extract_mesh",
    "tsdf_group_save_ply", "tsdf_group_save_mesh_ply", "tsdf_group_save_bin",
]
DIAG_SYMBOLS = [
    "tsdf_integrate_sequence_timed", "tsdf_integrate_frames_timed",
    "tsdf_probe_graph_replay", "tsdf_probe_stream",
    "tsdf_selftest_fastdiv", "tsdf_selftest_fastdiv_band", "tsdf_selftest_round", "tsdf_selftest_tile_tables",
    "tsdf_shortcut_stats", "tsdf_brick_list_stats", "tsdf_classification_info", "tsdf_store_stats", "tsdf_summary_stats", "tsdf_summary_words", "tsdf_frames_per_launch", "tsdf_last_cam2base",
    "tsdf_set_kernel_variant", "tsdf_set_brick_shape", "tsdf_brick_shape", "tsdf_default_brick_shape",
    "tsdf_scan_ground_tables",
]


class TsdfError(RuntimeError):
    pass


# kernel variants of the library as shipped (tsdf_set_kernel_variant; csrc/tsdf_capi.hip); every other number exists only in
# the measurement build (`make -C semantic_slam_amd/csrc experiments`, loaded through TSDF_HIP_LIB)
SHIPPED_VARIANTS = (0, 1, 3, 7, 8)


def experiments_build():
    """True when the loaded library is the measurement build (-DTSDF_EXPERIMENTS)."""
    return b"+experiments" in load().tsdf_version()


def variants(*wanted):
    """Those of `wanted` the loaded library knows: the shipped ones, and the experiments when that build is loaded (tests
    parametrise over this, so the product's test matrix is exactly what ships)."""
    exp = experiments_build()
    return [v for v in wanted if v in SHIPPED_VARIANTS or exp]


class TsdfConfig(C.Structure):
    """Mirror of `struct tsdf_config` (include/tsdf_hip.h)."""
    _fields_ = [
        ("im_height", C.c_int32), ("im_width", C.c_int32),
        ("dim_x", C.c_int32), ("dim_y", C.c_int32), ("dim_z", C.c_int32),
        ("z_begin", C.c_int32), ("z_end", C.c_int32),
        ("voxel_size", C.c_float), ("trunc_margin", C.c_float), ("max_depth", C.c_float),
        ("origin", C.c_float * 3), ("cam_K", C.c_float * 9), ("base2world", C.c_float * 16),
        ("device", C.c_int32), ("id", C.c_int32),
    ]


class RaycastParams(C.Structure):
    """Mirror of `struct tsdf_raycast_params` (include/tsdf_hip.h)."""
    _fields_ = [
        ("cam_K", C.c_float * 9), ("im_height", C.c_int32), ("im_width", C.c_int32),
        ("near_m", C.c_float), ("far_m", C.c_float), ("weight_thresh", C.c_float),
    ]


class TrackParams(C.Structure):
    """Mirror of `struct tsdf_track_params` (include/tsdf_hip.h)."""
    _fields_ = [
        ("ray", RaycastParams), ("n_levels", C.c_int32), ("iters", C.c_int32 * 3), ("dist_thresh", C.c_float * 3),
        ("cos_normal_thresh", C.c_float), ("min_inliers", C.c_int32), ("eps_rot", C.c_float), ("eps_trans", C.c_float),
    ]


class TrackResult(C.Structure):
    """Mirror of `struct tsdf_track_result` (include/tsdf_hip.h)."""
    _fields_ = [
        ("cam2world", C.c_float * 16), ("status", C.c_int32), ("iters_run", C.c_int32 * 3), ("inliers", C.c_int32),
        ("rmse", C.c_float),
    ]


class PhotoParams(C.Structure):
    """Mirror of `struct tsdf_photo_params` (include/tsdf_hip.h)."""
    _fields_ = [("photo_weight", C.c_float), ("intensity_thresh", C.c_float)]


class TrackRgbdResult(C.Structure):
    """Mirror of `struct tsdf_track_rgbd_result` (include/tsdf_hip.h)."""
    _fields_ = [("geo", TrackResult), ("photo_pairs", C.c_int32), ("photo_rmse", C.c_float)]


class FuseParams(C.Structure):
    """Mirror of `struct tsdf_fuse_params` (include/tsdf_hip.h)."""
    _fields_ = [("weight_thresh", C.c_float), ("agree_tol", C.c_float), ("write", C.c_int32)]


class FuseCounts(C.Structure):
    """Mirror of `struct tsdf_fuse_counts` (include/tsdf_hip.h)."""
    _fields_ = [("sampled", C.c_uint64), ("both", C.c_uint64), ("both_band", C.c_uint64), ("agree_band", C.c_uint64)]


FUSE_CARRY_COLOUR, FUSE_CARRY_LABELS = 1, 2      # TSDF_FUSE_CARRY_* (include/tsdf_hip.h)


class FuseCarryCounts(C.Structure):
    """Mirror of `struct tsdf_fuse_carry_counts` (include/tsdf_hip.h)."""
    _fields_ = [("label_adopted", C.c_uint64), ("label_agreed", C.c_uint64), ("label_opposed", C.c_uint64),
                ("label_flipped", C.c_uint64)]


class AlignParams(C.Structure):
    """Mirror of `struct tsdf_align_params` (include/tsdf_hip.h)."""
    _fields_ = [("weight_thresh", C.c_float), ("resid_thresh", C.c_float), ("n_levels", C.c_int32), ("iters", C.c_int32 * 3),
                ("min_pairs", C.c_int32), ("eps_rot", C.c_float), ("eps_trans", C.c_float)]


class AlignResult(C.Structure):
    """Mirror of `struct tsdf_align_result` (include/tsdf_hip.h)."""
    _fields_ = [("dst2src", C.c_float * 16), ("status", C.c_int32), ("iters_run", C.c_int32 * 3), ("pairs", C.c_int32),
                ("rmse", C.c_float)]


class ExtentParams(C.Structure):
    """Mirror of `struct tsdf_extent_params` (include/tsdf_hip.h)."""
    _fields_ = [("weight_thresh", C.c_float), ("band", C.c_float), ("margin", C.c_int32)]


class Extent(C.Structure):
    """Mirror of `struct tsdf_extent` (include/tsdf_hip.h): integers only."""
    _fields_ = [
        ("n_observed", C.c_uint64), ("n_surface", C.c_uint64), ("sum", C.c_uint64 * 3), ("sum2", C.c_uint64 * 6),
        ("border", C.c_uint64 * 6), ("lo", C.c_int32 * 3), ("hi", C.c_int32 * 3),
    ]

    def as_dict(self):
        """The record as plain Python integers (lists for the arrays): what tests/extent_spec.py produces."""
        return {"n_observed": int(self.n_observed), "n_surface": int(self.n_surface), "sum": [int(x) for x in self.sum],
                "sum2": [int(x) for x in self.sum2], "border": [int(x) for x in self.border], "lo": [int(x) for x in self.lo],
                "hi": [int(x) for x in self.hi]}

    @classmethod
    def from_dict(cls, d):
        e = cls()
        e.n_observed, e.n_surface = d["n_observed"], d["n_surface"]
        for name in ("sum", "sum2", "border", "lo", "hi"):
            getattr(e, name)[:] = d[name]
        return e


class ExtentMetric(C.Structure):
    """Mirror of `struct tsdf_extent_metric` (include/tsdf_hip.h): doubles."""
    _fields_ = [("centroid_base", C.c_double * 3), ("centroid_world", C.c_double * 3), ("cov_base", C.c_double * 6),
                ("lo_base", C.c_double * 3), ("hi_base", C.c_double * 3)]


class AssociateParams(C.Structure):
    """Mirror of `struct tsdf_associate_params` (include/tsdf_hip.h)."""
    _fields_ = [
        ("ray", RaycastParams), ("depth_tol_m", C.c_float), ("min_pixels", C.c_int32), ("min_iou", C.c_float),
        ("one_to_one", C.c_int32),
    ]


class AssociateLabels(C.Structure):
    """Mirror of `struct tsdf_associate_labels` (include/tsdf_hip.h): four host arrays."""
    _fields_ = [("mask_label", C.c_void_p), ("mask_score", C.c_void_p), ("member_label", C.c_void_p),
                ("member_score", C.c_void_p)]


class SegmentParams(C.Structure):
    """Mirror of `struct tsdf_segment_params` (include/tsdf_hip.h)."""
    _fields_ = [
        ("cam_K", C.c_float * 9), ("im_height", C.c_int32), ("im_width", C.c_int32), ("near_m", C.c_float), ("far_m", C.c_float),
        ("small_radius_m", C.c_float), ("large_radius_m", C.c_float), ("don_thresh", C.c_float), ("seg_radius_m", C.c_float),
        ("min_cluster", C.c_int32), ("max_cluster", C.c_int32), ("overlap", C.c_float), ("inset", C.c_int32),
    ]


class ScanFillParams(C.Structure):
    """Mirror of `struct tsdf_scan_fill_params` (include/tsdf_hip.h)."""
    _fields_ = [("max_span_u", C.c_int32), ("max_span_v", C.c_int32), ("jump_rel", C.c_float)]


class ScanGroundParams(C.Structure):
    """Mirror of `struct tsdf_scan_ground_params` (include/tsdf_hip.h)."""
    _fields_ = [("n_rings", C.c_int32), ("n_columns", C.c_int32), ("ang_res_y", C.c_float), ("ang_bottom", C.c_float),
                ("mount_deg", C.c_float), ("tol_deg", C.c_float), ("min_range", C.c_float), ("ground_rings", C.c_int32),
                ("mark_upper", C.c_int32)]


class ScanTrackParams(C.Structure):
    """Mirror of `struct tsdf_scan_track_params` (include/tsdf_hip.h)."""
    _fields_ = [("weight_thresh", C.c_float), ("resid_thresh", C.c_float), ("min_range_m", C.c_float), ("max_range_m", C.c_float),
                ("n_levels", C.c_int32), ("iters", C.c_int32 * 3), ("min_pairs", C.c_int32), ("drop_flag", C.c_int32),
                ("eps_rot", C.c_float), ("eps_trans", C.c_float)]


class ScanTrackResult(C.Structure):
    """Mirror of `struct tsdf_scan_track_result` (include/tsdf_hip.h)."""
    _fields_ = [("velo2world", C.c_float * 16), ("status", C.c_int32), ("iters_run", C.c_int32 * 3), ("pairs", C.c_int32),
                ("rmse", C.c_float)]


SCAN_DROP_GROUND, SCAN_ONLY_GROUND = 0, 1      # tsdf_scan_project_ground's and tsdf_integrate_scan_ground's `select`

TRACK_STATUS = {0: "converged", 1: "iterations exhausted", 2: "lost"}

_lib = None


def load():
    """Load libtsdf_hip.so (built by `make -C semantic_slam_amd/csrc` / __graft_entry__.build())."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.isfile(LIB_PATH):
        raise TsdfError(f"{LIB_PATH} not built: run `python -c 'import __graft_entry__ as g; g.build()'` "
                        "(there is no CPU fallback)")
    # One HIP runtime per process: PyTorch ships its own libamdhip64, this library links ROCm's.  Whichever is loaded
    # first serves both (same SONAME); loaded the other way round the process ends up with two runtimes, and the second
    # one to initialise sees no device (tsdf_create: "no HIP device visible").  Callers hand torch device pointers to this
    # library anyway, so torch -- when it is installed -- goes first.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    L = C.CDLL(LIB_PATH)
    vp, f32p, i64p = C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_int64)
    L.tsdf_config_default.argtypes = [C.POINTER(TsdfConfig), C.c_int32, C.c_int32]
    L.tsdf_create.argtypes = [C.POINTER(TsdfConfig), C.POINTER(vp)]
    L.tsdf_destroy.argtypes = [vp]
    L.tsdf_reset.argtypes = [vp]
    L.tsdf_integrate.argtypes = [vp, vp, vp]
    L.tsdf_set_deferral.argtypes = [vp, C.c_int32]
    L.tsdf_integrate_u16.argtypes = [vp, vp, C.c_float, C.c_int32, C.c_int32, vp]
    L.tsdf_convert_depth_u16.argtypes = [vp, vp, vp, C.c_float, C.c_int32, C.c_int32]
    L.tsdf_integrate_device.argtypes = [vp, vp, vp]
    L.tsdf_integrate_cam2base.argtypes = [vp, vp, vp]
    L.tsdf_integrate_masked_device.argtypes = [vp, vp, vp, vp]
    L.tsdf_integrate_frames_device.argtypes = [vp, vp, vp, vp, C.c_int32]
    L.tsdf_sync.argtypes = [vp]
    L.tsdf_download.argtypes = [vp, vp, vp]
    L.tsdf_upload.argtypes = [vp, vp, vp]
    L.tsdf_copy_slices.argtypes = [vp, C.c_int32, C.c_int32, vp, vp]
    L.tsdf_refresh_summary.argtypes = [vp]
    L.tsdf_device_ptrs.argtypes = [vp, C.POINTER(vp), C.POINTER(vp)]
    L.tsdf_slab_voxels.argtypes = [vp]
    L.tsdf_slab_voxels.restype = C.c_int64
    L.tsdf_frames_per_launch.argtypes = [vp]
    L.tsdf_frames_per_launch.restype = C.c_int32
    L.tsdf_shortcut_stats.argtypes = [vp, C.c_int32, vp]
    L.tsdf_classification_info.argtypes = [vp, vp]
    L.tsdf_brick_list_stats.argtypes = [vp, vp]
    if hasattr(L, "tsdf_store_stats"):      # (an earlier build loaded through TSDF_HIP_LIB for an A/B has none)
        L.tsdf_store_stats.argtypes = [vp, i64p]
    if hasattr(L, "tsdf_summary_stats"):    # (likewise)
        L.tsdf_summary_stats.argtypes = [vp, vp]
    if hasattr(L, "tsdf_summary_words"):    # (likewise)
        L.tsdf_summary_words.argtypes = [vp, vp, C.c_int64, i64p]
    L.tsdf_get_config.argtypes = [vp, C.POINTER(TsdfConfig)]
    L.tsdf_last_cam2base.argtypes = [vp, vp]
    L.tsdf_set_stream.argtypes = [vp, vp]
    L.tsdf_get_stream.argtypes = [vp, C.POINTER(vp)]
    L.tsdf_count_surface.argtypes = [vp, C.c_float, i64p]
    L.tsdf_extract_surface.argtypes = [vp, C.c_float, vp, C.c_int64, i64p]
    L.tsdf_extract_crossings.argtypes = [vp, vp, vp, C.c_float, vp, C.c_int64, i64p]
    L.tsdf_extract_mesh.argtypes = [vp, vp, vp, C.c_float, vp, C.c_int64, i64p]
    L.tsdf_save_mesh_ply.argtypes = [vp, C.c_char_p, C.c_float]
    L.tsdf_save_mesh_welded_ply.argtypes = [vp, C.c_char_p, C.c_float]
    L.tsdf_save_ply.argtypes = [vp, C.c_char_p, C.c_float]
    L.tsdf_save_bin.argtypes = [vp, C.c_char_p]
    L.tsdf_load_bin.argtypes = [vp, C.c_char_p]
    L.tsdf_save_state.argtypes = [vp, C.c_char_p]
    L.tsdf_load_state.argtypes = [vp, C.c_char_p]
    L.tsdf_integrate_sequence_timed.argtypes = [vp, vp, vp, C.c_int32, f32p]
    L.tsdf_integrate_frames_timed.argtypes = [vp, vp, vp, vp, C.c_int32, f32p]
    L.tsdf_probe_graph_replay.argtypes = [vp, vp, vp, C.c_int32, C.c_int32, f32p, f32p]
    L.tsdf_probe_stream.argtypes = [vp, C.c_int32, C.c_int32, f32p]
    L.tsdf_selftest_fastdiv.argtypes = [C.c_int32, C.c_uint64, C.c_uint64, C.c_float, C.c_float, C.POINTER(C.c_uint64), f32p]
    L.tsdf_selftest_fastdiv_band.argtypes = [C.c_int32, C.c_uint64, C.c_uint64, C.POINTER(C.c_uint64), f32p]
    L.tsdf_selftest_round.argtypes = [C.c_int32, C.POINTER(C.c_uint64), f32p]
    L.tsdf_selftest_tile_tables.argtypes = [C.c_int32, vp, vp, C.c_int32, C.c_int32, C.c_float, C.POINTER(C.c_uint64)]
    L.tsdf_set_kernel_variant.argtypes = [vp, C.c_int32]
    L.tsdf_set_brick_shape.argtypes = [vp, C.c_int32, C.c_int32, C.c_int32]
    L.tsdf_brick_shape.argtypes = [vp, C.POINTER(C.c_int32)]
    L.tsdf_default_brick_shape.argtypes = [C.POINTER(TsdfConfig), C.POINTER(C.c_int32)]
    L.tsdf_last_error.restype = C.c_char_p
    L.tsdf_version.restype = C.c_char_p
    L.tsdf_multiply_matrix.argtypes = [vp, vp, vp]
    L.tsdf_multiply_matrix.restype = None
    L.tsdf_invert_matrix.argtypes = [vp, vp]
    L.tsdf_labels_enable.argtypes = [vp, C.c_float]
    L.tsdf_compose_labels.argtypes = [vp, vp, vp, vp, C.c_int32, vp, vp]
    L.tsdf_integrate_labels_device.argtypes = [vp, vp, vp, vp, vp]
    L.tsdf_download_labels.argtypes = [vp, vp, vp, vp]
    L.tsdf_integrate_frames_labels_device.argtypes = [vp, vp, vp, vp, vp, C.c_int32]
    L.tsdf_colour_enable.argtypes = [vp]
    L.tsdf_integrate_colour_device.argtypes = [vp, vp, vp, vp]
    L.tsdf_integrate_rgbd.argtypes = [vp, vp, vp, vp]
    L.tsdf_download_colour.argtypes = [vp, vp]
    L.tsdf_raycast_params_default.argtypes = [C.POINTER(TsdfConfig), C.POINTER(RaycastParams)]
    L.tsdf_raycast_device.argtypes = [vp, C.POINTER(RaycastParams), vp, vp, vp, vp, vp]
    L.tsdf_raycast.argtypes = [vp, C.POINTER(RaycastParams), vp, vp, vp, vp, vp]
    L.tsdf_batch_raycast_device.argtypes = [vp, C.POINTER(RaycastParams), vp, vp, vp, vp]
    L.tsdf_track_params_default.argtypes = [C.POINTER(TsdfConfig), C.POINTER(TrackParams)]
    L.tsdf_track.argtypes = [vp, C.POINTER(TrackParams), vp, vp, vp, C.POINTER(TrackResult)]
    L.tsdf_track_system.argtypes = [vp, C.POINTER(TrackParams), vp, vp, vp, vp, C.c_int32, vp]
    L.tsdf_photo_params_default.argtypes = [C.POINTER(TsdfConfig), C.POINTER(PhotoParams)]
    L.tsdf_track_rgbd.argtypes = [vp, C.POINTER(TrackParams), C.POINTER(PhotoParams), vp, vp, vp, vp, C.POINTER(TrackRgbdResult)]
    L.tsdf_track_rgbd_system.argtypes = [vp, C.POINTER(TrackParams), C.POINTER(PhotoParams), vp, vp, vp, vp, vp, C.c_int32, vp, vp]
    L.tsdf_render_intensity.argtypes = [vp, C.POINTER(RaycastParams), vp, C.c_int32, vp]
    L.tsdf_batch_track.argtypes = [vp, C.POINTER(TrackParams), vp, vp, vp, vp, C.POINTER(TrackResult), vp]
    L.tsdf_batch_track_system.argtypes = [vp, C.POINTER(TrackParams), vp, vp, vp, vp, C.c_int32, vp]
    L.tsdf_track_member_systems.argtypes = [C.c_int32, C.POINTER(TrackParams), vp, vp, vp, C.c_int32, vp, vp, vp, vp,
                                            C.c_int32, vp]
    L.tsdf_fuse_params_default.argtypes = [C.POINTER(TsdfConfig), C.POINTER(FuseParams)]
    L.tsdf_fuse_volume.argtypes = [vp, vp, C.POINTER(FuseParams), C.POINTER(FuseCounts)]
    L.tsdf_align_params_default.argtypes = [C.POINTER(TsdfConfig), C.POINTER(AlignParams)]
    L.tsdf_fuse_pose_default.argtypes = [C.POINTER(TsdfConfig), C.POINTER(TsdfConfig), vp]
    L.tsdf_align_volume.argtypes = [vp, vp, C.POINTER(AlignParams), vp, C.POINTER(AlignResult)]
    L.tsdf_align_system.argtypes = [vp, vp, C.POINTER(AlignParams), vp, C.c_int32, vp]
    L.tsdf_fuse_volume_at.argtypes = [vp, vp, C.POINTER(FuseParams), vp, C.POINTER(FuseCounts)]
    if hasattr(L, "tsdf_fuse_volume_carry"):    # (an earlier build loaded through TSDF_HIP_LIB for an A/B has none)
        L.tsdf_fuse_volume_carry.argtypes = [vp, vp, C.POINTER(FuseParams), vp, C.c_uint32, C.POINTER(FuseCounts),
                                             C.POINTER(FuseCarryCounts)]
        L.tsdf_upload_labels.argtypes = [vp, vp, vp, vp]
        L.tsdf_upload_colour.argtypes = [vp, vp]
    L.tsdf_extent_params_default.argtypes = [C.POINTER(TsdfConfig), C.POINTER(ExtentParams)]
    L.tsdf_volume_extent.argtypes = [vp, C.POINTER(ExtentParams), C.POINTER(Extent)]
    L.tsdf_batch_extents.argtypes = [vp, C.POINTER(ExtentParams), C.POINTER(Extent)]
    L.tsdf_group_extent.argtypes = [vp, C.POINTER(ExtentParams), C.POINTER(Extent)]
    L.tsdf_extent_combine.argtypes = [C.POINTER(Extent), C.POINTER(Extent), C.POINTER(Extent)]
    L.tsdf_extent_metric.argtypes = [C.POINTER(TsdfConfig), C.POINTER(Extent), C.POINTER(ExtentMetric)]
    L.tsdf_extent_regrid.argtypes = [C.POINTER(TsdfConfig), C.POINTER(Extent), C.c_int32, C.c_int32, C.POINTER(TsdfConfig)]
    L.tsdf_associate_params_default.argtypes = [C.POINTER(TsdfConfig), C.POINTER(AssociateParams)]
    L.tsdf_associate_count.argtypes = [C.c_int32, C.POINTER(AssociateParams), vp, vp, C.c_int32, vp, vp, C.c_int32, vp]
    L.tsdf_associate_assign.argtypes = [C.POINTER(AssociateParams), vp, C.c_int32, C.c_int32, C.POINTER(AssociateLabels), vp,
                                        vp]
    L.tsdf_batch_associate.argtypes = [vp, C.POINTER(AssociateParams), vp, vp, vp, C.c_int32, C.POINTER(AssociateLabels),
                                       vp, vp, vp]
    L.tsdf_segment_params_default.argtypes = [C.POINTER(TsdfConfig), C.POINTER(SegmentParams)]
    L.tsdf_segmenter_create.argtypes = [C.c_int32, C.c_int32, C.c_int32, C.POINTER(vp)]
    L.tsdf_segmenter_destroy.argtypes = [vp]
    L.tsdf_segmenter_set_stream.argtypes = [vp, vp]
    L.tsdf_segment_depth_device.argtypes = [vp, C.POINTER(SegmentParams), vp, vp, vp, C.POINTER(C.c_int32)]
    L.tsdf_segment_refine_masks_device.argtypes = [vp, C.POINTER(SegmentParams), vp, C.c_int32, vp, C.c_int32, vp, vp]
    L.tsdf_segment_frame.argtypes = [vp, C.POINTER(SegmentParams), vp, vp, C.c_int32, vp, vp, C.POINTER(C.c_int32)]
    L.tsdf_scan_projection.argtypes = [vp, vp, vp, vp, vp]
    L.tsdf_scanner_create.argtypes = [C.c_int32, C.c_int32, C.c_int32, C.POINTER(vp)]
    L.tsdf_scanner_destroy.argtypes = [vp]
    L.tsdf_scan_project.argtypes = [vp, vp, vp, vp, C.c_int64, vp, vp, i64p]
    L.tsdf_scan_range_to_depth.argtypes = [vp, vp, vp, vp]
    L.tsdf_integrate_range.argtypes = [vp, vp, vp]
    L.tsdf_integrate_scan.argtypes = [vp, vp, vp, C.c_int64, vp]
    L.tsdf_scan_fill_params_default.argtypes = [vp]
    L.tsdf_scan_fill_depth.argtypes = [vp, vp, vp, vp, vp, i64p]
    L.tsdf_scan_project_filled.argtypes = [vp, vp, vp, vp, vp, C.c_int64, vp, vp, i64p]
    L.tsdf_integrate_range_filled.argtypes = [vp, vp, vp, vp]
    L.tsdf_integrate_scan_filled.argtypes = [vp, vp, vp, vp, C.c_int64, vp]
    L.tsdf_scan_ground_params_default.argtypes = [vp]
    L.tsdf_scan_mark_ground.argtypes = [vp, vp, vp, C.c_int64, vp, vp, vp, vp]
    L.tsdf_scan_project_ground.argtypes = [vp, vp, vp, vp, C.c_int32, vp, vp, C.c_int64, vp, vp, vp, i64p, i64p, i64p]
    L.tsdf_integrate_scan_ground.argtypes = [vp, vp, vp, C.c_int32, vp, vp, C.c_int64, vp]
    L.tsdf_scan_ground_tables.argtypes = [vp, vp, vp, vp, vp, vp, vp]
    L.tsdf_scan_track_params_default.argtypes = [C.POINTER(TsdfConfig), C.POINTER(ScanTrackParams)]
    L.tsdf_scan_pose.argtypes = [vp, vp, vp, vp]
    L.tsdf_scan_track.argtypes = [vp, C.POINTER(ScanTrackParams), vp, C.c_int64, vp, vp, C.POINTER(ScanTrackResult)]
    L.tsdf_scan_track_system.argtypes = [vp, C.POINTER(ScanTrackParams), vp, C.c_int64, vp, vp, C.c_int32, vp]
    L.tsdf_object_origin.argtypes = [C.c_int32, vp, vp, C.c_int32, C.c_int32, vp, vp]
    L.tsdf_batch_create.argtypes = [C.POINTER(TsdfConfig), C.c_int32, C.POINTER(vp)]
    L.tsdf_batch_destroy.argtypes = [vp]
    L.tsdf_batch_size.argtypes = [vp]
    L.tsdf_batch_volume.argtypes = [vp, C.c_int32, C.POINTER(vp)]
    L.tsdf_batch_integrate_device.argtypes = [vp, vp, vp, vp]
    L.tsdf_batch_sync.argtypes = [vp]
    L.tsdf_group_create.argtypes = [C.POINTER(TsdfConfig), C.POINTER(C.c_int32), C.c_int32, C.POINTER(vp)]
    L.tsdf_group_destroy.argtypes = [vp]
    L.tsdf_group_size.argtypes = [vp]
    L.tsdf_group_voxels.argtypes = [vp]
    L.tsdf_group_voxels.restype = C.c_int64
    L.tsdf_group_volume.argtypes = [vp, C.c_int32, C.POINTER(vp)]
    L.tsdf_group_integrate.argtypes = [vp, vp, vp]
    L.tsdf_group_integrate_frames.argtypes = [vp, vp, vp, C.c_int32]
    L.tsdf_group_set_deferral.argtypes = [vp, C.c_int32]
    L.tsdf_group_sync.argtypes = [vp]
    L.tsdf_group_reset.argtypes = [vp]
    L.tsdf_group_download.argtypes = [vp, vp, vp]
    for name in ("tsdf_group_extract_surface", "tsdf_group_extract_crossings", "tsdf_group_extract_mesh"):
        getattr(L, name).argtypes = [vp, C.c_float, vp, C.c_int64, i64p]
    L.tsdf_group_save_ply.argtypes = [vp, C.c_char_p, C.c_float]
    L.tsdf_group_save_mesh_ply.argtypes = [vp, C.c_char_p, C.c_float]
    L.tsdf_group_save_bin.argtypes = [vp, C.c_char_p]
    _lib = L
    return L


def check(rc, what=""):
    if rc != 0:
        raise TsdfError(f"{what} failed ({rc}): {load().tsdf_last_error().decode()}")


def _f32(a, n=None):
    a = np.ascontiguousarray(a, dtype=np.float32).ravel()
    if n is not None and a.size != n:
        raise ValueError(f"expected {n} floats, got {a.size}")
    return a


def default_config(im_height=480, im_width=640):
    cfg = TsdfConfig()
    check(load().tsdf_config_default(C.byref(cfg), im_height, im_width), "tsdf_config_default")
    return cfg


def make_config(dims, voxel_size, origin, trunc=None, K=None, base2world=None, z_begin=0, z_end=None,
                im_height=480, im_width=640, max_depth=None, device=0, vol_id=0):
    """Reference defaults (include/tsdf.hpp:63-67,96) with the given overrides."""
    cfg = default_config(im_height, im_width)
    cfg.dim_x, cfg.dim_y, cfg.dim_z = (int(d) for d in dims)
    cfg.z_begin = int(z_begin)
    cfg.z_end = int(cfg.dim_z if z_end is None else z_end)
    cfg.voxel_size = voxel_size
    # the reference's member initialiser: trunc_margin = voxel_size * 5 in fp32
    cfg.trunc_margin = float(np.float32(voxel_size) * np.float32(5)) if trunc is None else trunc
    if max_depth is not None:
        cfg.max_depth = max_depth
    cfg.origin[:] = [float(x) for x in _f32(origin, 3)]
    if K is not None:
        cfg.cam_K[:] = [float(x) for x in _f32(K, 9)]
    if base2world is not None:
        cfg.base2world[:] = [float(x) for x in _f32(base2world, 16)]
    cfg.device = device
    cfg.id = vol_id
    return cfg


def multiply_matrix(a, b):
    out = np.empty(16, np.float32)
    a, b = _f32(a, 16), _f32(b, 16)
    load().tsdf_multiply_matrix(a.ctypes.data, b.ctypes.data, out.ctypes.data)
    return out


def invert_matrix(m):
    out = np.zeros(16, np.float32)
    m = _f32(m, 16)
    ok = load().tsdf_invert_matrix(m.ctypes.data, out.ctypes.data)
    return bool(ok), out


def selftest_fastdiv(n_samples, seed=1, device=0, fx=535.4, cx=320.1):
    """Returns (mismatches, first_bad[4]) of the device division self-test."""
    cnt = C.c_uint64()
    bad = (C.c_float * 4)()
    check(load().tsdf_selftest_fastdiv(device, seed, n_samples, fx, cx, C.byref(cnt), bad), "tsdf_selftest_fastdiv")
    return cnt.value, list(bad)


def selftest_fastdiv_band(n_samples, seed=1, device=0):
    """Returns (mismatches, first_bad[4]) of the device self-test of diff / trunc through the shared reciprocal."""
    cnt = C.c_uint64()
    bad = (C.c_float * 4)()
    check(load().tsdf_selftest_fastdiv_band(device, seed, n_samples, C.byref(cnt), bad), "tsdf_selftest_fastdiv_band")
    return cnt.value, list(bad)


def object_origin(depth_ptr, mask_ptr, h, w, K, device=0):
    """Origin of a new object volume from its first masked depth frame (ref: src/Object.cpp:37-49), on the device."""
    k = _f32(K, 9)
    out = np.empty(3, np.float32)
    check(load().tsdf_object_origin(device, depth_ptr, mask_ptr, h, w, k.ctypes.data, out.ctypes.data), "tsdf_object_origin")
    return out


def raycast_params_default(cfg):
    """Raycast parameters from a config: its K and image size, near 0, far = max_depth, weight_thresh 0.9 (no device)."""
    p = RaycastParams()
    check(load().tsdf_raycast_params_default(C.byref(cfg), C.byref(p)), "tsdf_raycast_params_default")
    return p


def track_params_default(cfg):
    """Tracking parameters from a config (include/tsdf_hip.h): raycast_params_default(cfg), 3 levels, iterations
    {10, 5, 4}, 0.10 m, cos(20 deg), min_inliers 300, eps 1e-5 rad / 1e-5 m (no device)."""
    p = TrackParams()
    check(load().tsdf_track_params_default(C.byref(cfg), C.byref(p)), "tsdf_track_params_default")
    return p


def photo_params_default(cfg):
    """Photometric tracking parameters (include/tsdf_hip.h): photo_weight 0.1, intensity_thresh 0.25 (no device)."""
    p = PhotoParams()
    check(load().tsdf_photo_params_default(C.byref(cfg), C.byref(p)), "tsdf_photo_params_default")
    return p


def fuse_params_default(cfg):
    """Merge parameters for a destination config (include/tsdf_hip.h): weight_thresh 0.9, agree_tol 0.4, write 1 (no
    device)."""
    p = FuseParams()
    check(load().tsdf_fuse_params_default(C.byref(cfg), C.byref(p)), "tsdf_fuse_params_default")
    return p


def align_params_default(cfg):
    """Registration parameters for a destination config (include/tsdf_hip.h): weight_thresh 0.9, resid_thresh 1.0, 2 levels,
    iterations {10, 10, 0}, min_pairs 300, eps 1e-5 rad / 1e-5 m (no device)."""
    p = AlignParams()
    check(load().tsdf_align_params_default(C.byref(cfg), C.byref(p)), "tsdf_align_params_default")
    return p


def fuse_pose_default(dst_cfg, src_cfg):
    """The pose tsdf_fuse_volume composes from two configs: inverse(base2world_src) * base2world_dst, float32 [16] (no
    device)."""
    out = np.empty(16, np.float32)
    check(load().tsdf_fuse_pose_default(C.byref(dst_cfg), C.byref(src_cfg), out.ctypes.data), "tsdf_fuse_pose_default")
    return out


def extent_params_default(cfg):
    """Extent parameters from a config (include/tsdf_hip.h): weight_thresh 0.9, band 1.0, margin = ceil(trunc_margin /
    voxel_size) voxels (no device)."""
    p = ExtentParams()
    check(load().tsdf_extent_params_default(C.byref(cfg), C.byref(p)), "tsdf_extent_params_default")
    return p


def extent_combine(a, b):
    """The record of two disjoint sets of voxels of one grid (slabs) from the records of each (host only)."""
    out = Extent()
    check(load().tsdf_extent_combine(C.byref(a), C.byref(b), C.byref(out)), "tsdf_extent_combine")
    return out


def extent_metric(cfg, extent):
    """Metric form of a record (host only, double): dict of centroid_base [3], centroid_world [3], cov_base [6] (xx, yy, zz,
    xy, xz, yz), lo_base [3], hi_base [3] (the outer corners of the bounding voxels)."""
    m = ExtentMetric()
    check(load().tsdf_extent_metric(C.byref(cfg), C.byref(extent), C.byref(m)), "tsdf_extent_metric")
    return {name: np.array(getattr(m, name), np.float64) for name, _ in ExtentMetric._fields_}


def extent_regrid(cfg, extent, pad_voxels, dim_multiple=4):
    """The config of the grid to move an object into (host only): the record's bounds padded by pad_voxels, dims rounded up to
    a multiple of dim_multiple (batches need 4), whole-grid slab."""
    out = TsdfConfig()
    check(load().tsdf_extent_regrid(C.byref(cfg), C.byref(extent), pad_voxels, dim_multiple, C.byref(out)), "tsdf_extent_regrid")
    return out


def track_member_systems(params, model_depth_ptr, model_normal_ptr, member_ptr, n_members, depth_ptr, ref_cam2world,
                         cam2world, level=0, mask_ptr=None, device=0):
    """The member pass of joint tracking over caller images (device pointers): float64 [n_members, 29], row m the system of
    the pairs whose model pixel shows member m (tsdf_track_system's layout), at `level`, the model at ref_cam2world, the pairs
    at cam2world (tsdf_track_member_systems)."""
    ref, cur = _f32(ref_cam2world, 16), _f32(cam2world, 16)
    out = np.zeros((n_members, 29), np.float64)
    check(load().tsdf_track_member_systems(device, C.byref(params), model_depth_ptr, model_normal_ptr, member_ptr, n_members,
                                           depth_ptr, mask_ptr, ref.ctypes.data, cur.ctypes.data, level, out.ctypes.data),
          "tsdf_track_member_systems")
    return out


def associate_params_default(cfg):
    """Association parameters from a config (include/tsdf_hip.h): raycast_params_default(cfg), depth_tol_m = trunc_margin,
    min_pixels 25, min_iou 0.25, one_to_one 1 (no device)."""
    p = AssociateParams()
    check(load().tsdf_associate_params_default(C.byref(cfg), C.byref(p)), "tsdf_associate_params_default")
    return p


def associate_split(counts, k, n_members):
    """The three count arrays of a block, as views: overlap [k, M, 3] (agree, front, behind), mask [k, 3] (in mask, and live
    valid, and not rendered), member [M, 4] (agree, front, behind, live not valid)."""
    n_ov = 3 * k * n_members
    return (counts[:n_ov].reshape(k, n_members, 3), counts[n_ov:n_ov + 3 * k].reshape(k, 3),
            counts[n_ov + 3 * k:].reshape(n_members, 4))


def _associate_labels(labels):
    """(mask_label, mask_score, member_label, member_score) -> the C block and the arrays it points into (kept alive)."""
    if labels is None:
        return None, ()
    arrs = (np.ascontiguousarray(labels[0], np.uint16), np.ascontiguousarray(labels[1], np.float32),
            np.ascontiguousarray(labels[2], np.uint16), np.ascontiguousarray(labels[3], np.float32))
    return C.byref(AssociateLabels(*[a.ctypes.data for a in arrs])), arrs


def associate_count(params, member_ptr, rdepth_ptr, n_members, depth_ptr, masks_ptr, k, device=0):
    """Counts of the association rule over caller images (device pointers); returns (block, overlap, mask, member)."""
    counts = np.empty(3 * k * n_members + 3 * k + 4 * n_members, np.uint32)
    check(load().tsdf_associate_count(device, C.byref(params), member_ptr, rdepth_ptr, n_members, depth_ptr, masks_ptr, k,
                                      counts.ctypes.data), "tsdf_associate_count")
    return (counts,) + associate_split(counts, k, n_members)


def associate_assign(params, counts, k, n_members, labels=None):
    """The assignment on a count block (host only); labels: None or (mask_label, mask_score, member_label, member_score).
    Returns (assign int32 [k], iou float32 [k])."""
    counts = np.ascontiguousarray(counts, np.uint32)
    if counts.size != 3 * k * n_members + 3 * k + 4 * n_members:
        raise ValueError(f"a block of {counts.size} words does not fit k = {k}, n_members = {n_members}")
    lab, keep = _associate_labels(labels)
    assign, iou = np.empty(k, np.int32), np.empty(k, np.float32)
    check(load().tsdf_associate_assign(C.byref(params), counts.ctypes.data, k, n_members, lab, assign.ctypes.data,
                                       iou.ctypes.data), "tsdf_associate_assign")
    del keep
    return assign, iou


def segment_params_default(cfg):
    """Segmentation parameters from a config (include/tsdf_hip.h): its K and image size, near 0, far = max_depth, radii 0.05 /
    0.5 m, don_thresh 0.1, seg_radius 0.05 m, clusters of 15..1000000 pixels, overlap 0.5, inset 2 (no device)."""
    p = SegmentParams()
    check(load().tsdf_segment_params_default(C.byref(cfg), C.byref(p)), "tsdf_segment_params_default")
    return p


def segment_split(counts, n_clusters, k):
    """The two count arrays of a refinement block, as views: size [C], inside [C, k]."""
    return counts[:n_clusters], counts[n_clusters:].reshape(n_clusters, k)


class Segmenter:
    """A tsdf_segmenter: geometric segmentation of depth frames of one size on one device and the refinement of instance
    masks by it.  Every argument named *_ptr is a device pointer; every call returns when its outputs are written."""

    def __init__(self, im_height, im_width, device=0):
        self.lib = load()
        self.h, self.w = int(im_height), int(im_width)
        self._h = C.c_void_p()
        check(self.lib.tsdf_segmenter_create(device, self.h, self.w, C.byref(self._h)), "tsdf_segmenter_create")

    def close(self):
        if self._h:
            self.lib.tsdf_segmenter_destroy(self._h)
            self._h = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_stream(self, hip_stream):
        """Queue on the caller's stream (a hipStream_t as an integer; None or 0: the segmenter's own again)."""
        check(self.lib.tsdf_segmenter_set_stream(self._h, hip_stream or None), "tsdf_segmenter_set_stream")

    def segment_depth(self, params, depth_ptr, cluster_ptr, don_ptr=None):
        """DoN and clusters of a depth frame into cluster_ptr (int32 [h, w]) and, unless None, don_ptr (float32 [h, w]);
        returns the number of clusters."""
        n = C.c_int32()
        check(self.lib.tsdf_segment_depth_device(self._h, C.byref(params), depth_ptr, don_ptr, cluster_ptr, C.byref(n)),
              "tsdf_segment_depth_device")
        return n.value

    def refine_masks(self, params, cluster_ptr, n_clusters, masks_ptr, k, masks_out_ptr, want_counts=True):
        """Refines k masks (uint8 [k, h, w]) by a cluster image with labels 0..n_clusters into masks_out_ptr; returns the
        count block (size [C], inside [C, k]) or None."""
        counts = np.zeros(n_clusters + n_clusters * k, np.uint32) if want_counts else None
        check(self.lib.tsdf_segment_refine_masks_device(self._h, C.byref(params), cluster_ptr, n_clusters, masks_ptr, k,
                                                        masks_out_ptr, counts.ctypes.data if want_counts else None),
              "tsdf_segment_refine_masks_device")
        return segment_split(counts, n_clusters, k) if want_counts else None

    def segment_frame(self, params, depth_ptr, masks_ptr, k, masks_out_ptr, cluster_ptr=None):
        """The product call: clusters of the frame, then the k masks refined by them; returns the number of clusters."""
        n = C.c_int32()
        check(self.lib.tsdf_segment_frame(self._h, C.byref(params), depth_ptr, masks_ptr, k, masks_out_ptr, cluster_ptr,
                                          C.byref(n)), "tsdf_segment_frame")
        return n.value


def scan_projection(P_rect, R_rect, R_velo, t_velo):
    """velo2img [3, 4] = P_rect * [R_rect 0; 0 1] * [R_velo t_velo; 0 1] in the library's fp32 operation order (no device)."""
    out = np.zeros(12, np.float32)
    P, Rr, Rv, t = _f32(P_rect, 12), _f32(R_rect, 9), _f32(R_velo, 9), _f32(t_velo, 3)
    check(load().tsdf_scan_projection(P.ctypes.data, Rr.ctypes.data, Rv.ctypes.data, t.ctypes.data, out.ctypes.data),
          "tsdf_scan_projection")
    return out.reshape(3, 4)


def scan_fill_params_default():
    """The gap fill's default parameters (include/tsdf_hip.h): max_span_u 5, max_span_v 8, jump_rel 0.05 (no device)."""
    p = ScanFillParams()
    check(load().tsdf_scan_fill_params_default(C.byref(p)), "tsdf_scan_fill_params_default")
    return p


def _scan_fill_params(params):
    """ScanFillParams from None (the defaults), a ScanFillParams or (max_span_u, max_span_v, jump_rel)."""
    if params is None:
        return scan_fill_params_default()
    if isinstance(params, ScanFillParams):
        return params
    su, sv, jump = params
    return ScanFillParams(int(su), int(sv), float(jump))


def scan_ground_params_default():
    """The ground marking's default parameters, the reference's literals (include/tsdf_hip.h): 64 x 4500 cells, 26.9 / 63 degrees
    per ring from -15.1, level within 0 +- 2.5 degrees, ranges from 0.1, 63 ring pairs, the upper cell not marked (no device)."""
    p = ScanGroundParams()
    check(load().tsdf_scan_ground_params_default(C.byref(p)), "tsdf_scan_ground_params_default")
    return p


def _scan_ground_params(params):
    """ScanGroundParams from None (the defaults), a ScanGroundParams, a dict of its fields over the defaults or the nine values."""
    if params is None:
        return scan_ground_params_default()
    if isinstance(params, ScanGroundParams):
        return params
    if isinstance(params, dict):
        p = scan_ground_params_default()
        for k, v in params.items():
            if k not in dict(ScanGroundParams._fields_):
                raise ValueError(f"tsdf_scan_ground_params has no field {k}")
            setattr(p, k, v)
        return p
    nr, nc, res, bottom, mount, tol, min_range, rings, upper = params
    return ScanGroundParams(int(nr), int(nc), float(res), float(bottom), float(mount), float(tol), float(min_range), int(rings), int(upper))


def scan_ground_tables(params=None):
    """The tables the library searches under these parameters (tsdf_scan_ground_tables; no device): {"T": [n_rings + 1],
    "C", "S": [n_columns], "tlo", "thi": float32, "first", "len": [4] int32 -- the quadrants' runs of column boundaries}."""
    p = _scan_ground_params(params)
    if not (0 < p.n_rings <= 1 << 20 and 0 < p.n_columns <= 1 << 20):
        raise TsdfError(f"tsdf_scan_ground_tables: n_rings = {p.n_rings}, n_columns = {p.n_columns}")
    T, Cc, S = np.zeros(p.n_rings + 1, np.float32), np.zeros(p.n_columns, np.float32), np.zeros(p.n_columns, np.float32)
    slopes, first, length = np.zeros(2, np.float32), np.zeros(4, np.int32), np.zeros(4, np.int32)
    check(load().tsdf_scan_ground_tables(C.addressof(p), T.ctypes.data, Cc.ctypes.data, S.ctypes.data, slopes.ctypes.data,
                                         first.ctypes.data, length.ctypes.data), "tsdf_scan_ground_tables")
    return {"T": T, "C": Cc, "S": S, "tlo": slopes[0], "thi": slopes[1], "first": first, "len": length}


def _scan_points(points):
    """A scan as contiguous float32 [n, 4] (the KITTI .bin layout)."""
    pts = np.ascontiguousarray(points, dtype=np.float32)
    if pts.ndim != 2 or pts.shape[1] != 4:
        raise ValueError(f"expected points of shape [n, 4], got {pts.shape}")
    return pts


def scan_track_params_default(cfg):
    """Scan tracking parameters for a volume's config (include/tsdf_hip.h): weight_thresh 0.9, resid_thresh = the truncation
    distance, ranges 2.5 ... 80 m, 3 levels of {10, 5, 4} iterations, min_pairs 300, drop_flag -1, eps 1e-5 rad / 1e-5 m
    (no device)."""
    p = ScanTrackParams()
    check(load().tsdf_scan_track_params_default(C.byref(cfg), C.byref(p)), "tsdf_scan_track_params_default")
    return p


def scan_pose(R_rect, R_velo, t_velo):
    """velo2cam [4, 4] = [R_rect 0; 0 1] * [R_velo t_velo; 0 1] in the library's fp32 operation order (no device)."""
    out = np.zeros(16, np.float32)
    Rr, Rv, t = _f32(R_rect, 9), _f32(R_velo, 9), _f32(t_velo, 3)
    check(load().tsdf_scan_pose(Rr.ctypes.data, Rv.ctypes.data, t.ctypes.data, out.ctypes.data), "tsdf_scan_pose")
    return out.reshape(4, 4)


def _scan_flags(flags, n):
    """A scan's flags as contiguous uint8 [n], or None."""
    if flags is None:
        return None
    f = np.ascontiguousarray(flags, dtype=np.uint8).ravel()
    if f.size != n:
        raise ValueError(f"expected {n} flags, got {f.size}")
    return f


class Scanner:
    """A tsdf_scanner: lidar scans into range and z-depth images of one size on one device.  Every array is host memory;
    every call returns with its outputs written."""

    def __init__(self, im_height, im_width, device=0):
        self.lib = load()
        self.h, self.w = int(im_height), int(im_width)
        self._h = C.c_void_p()
        check(self.lib.tsdf_scanner_create(device, self.h, self.w, C.byref(self._h)), "tsdf_scanner_create")

    def close(self):
        if self._h:
            self.lib.tsdf_scanner_destroy(self._h)
            self._h = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def project(self, points, velo2img, K=None, want_range=True, want_depth=True, want_count=True):
        """(range [h, w] or None, depth [h, w] or None, written pixels or None) of a scan [n, 4]; K is needed for the depth."""
        pts = _scan_points(points)
        m = _f32(velo2img, 12)
        k = None if K is None else _f32(K, 9)
        rng = np.empty((self.h, self.w), np.float32) if want_range else None
        dep = np.empty((self.h, self.w), np.float32) if want_depth else None
        n = C.c_int64(-1)
        check(self.lib.tsdf_scan_project(self._h, m.ctypes.data, None if k is None else k.ctypes.data,
                                         pts.ctypes.data if len(pts) else None, len(pts),
                                         None if rng is None else rng.ctypes.data, None if dep is None else dep.ctypes.data,
                                         C.byref(n) if want_count else None), "tsdf_scan_project")
        return rng, dep, (int(n.value) if want_count else None)

    def range_to_depth(self, range_im, K):
        """The z-depth image of a range image [h, w] under the camera K."""
        r = np.ascontiguousarray(range_im, dtype=np.float32)
        if r.shape != (self.h, self.w):
            raise ValueError(f"the range image is {r.shape}, the scanner's {(self.h, self.w)}")
        k = _f32(K, 9)
        out = np.empty((self.h, self.w), np.float32)
        check(self.lib.tsdf_scan_range_to_depth(self._h, k.ctypes.data, r.ctypes.data, out.ctypes.data), "tsdf_scan_range_to_depth")
        return out

    def fill_depth(self, depth, params=None, want_depth=True, want_kind=True, want_count=True, in_place=False):
        """(filled depth [h, w] or None, kind [h, w] uint8 or None, filled pixels or None) of a sparse z-depth image [h, w];
        in_place writes the filled image over `depth` itself (a contiguous float32 array)."""
        d = depth if in_place else np.ascontiguousarray(depth, dtype=np.float32)
        if in_place and not (isinstance(d, np.ndarray) and d.dtype == np.float32 and d.flags["C_CONTIGUOUS"] and want_depth):
            raise ValueError("in_place needs a contiguous float32 array and want_depth")
        if d.shape != (self.h, self.w):
            raise ValueError(f"the depth image is {d.shape}, the scanner's {(self.h, self.w)}")
        p = _scan_fill_params(params)
        out = d if in_place else (np.empty((self.h, self.w), np.float32) if want_depth else None)
        kind = np.empty((self.h, self.w), np.uint8) if want_kind else None
        n = C.c_int64(-1)
        check(self.lib.tsdf_scan_fill_depth(self._h, C.addressof(p), d.ctypes.data, None if out is None else out.ctypes.data,
                                            None if kind is None else kind.ctypes.data, C.byref(n) if want_count else None),
              "tsdf_scan_fill_depth")
        return out, kind, (int(n.value) if want_count else None)

    def project_filled(self, points, velo2img, K, params=None, want_depth=True, want_kind=True, want_count=True):
        """project()'s depth image through fill_depth() without leaving the device: (filled depth, kind, filled pixels)."""
        pts = _scan_points(points)
        m, k = _f32(velo2img, 12), _f32(K, 9)
        p = _scan_fill_params(params)
        dep = np.empty((self.h, self.w), np.float32) if want_depth else None
        kind = np.empty((self.h, self.w), np.uint8) if want_kind else None
        n = C.c_int64(-1)
        check(self.lib.tsdf_scan_project_filled(self._h, m.ctypes.data, k.ctypes.data, C.addressof(p),
                                                pts.ctypes.data if len(pts) else None, len(pts),
                                                None if dep is None else dep.ctypes.data, None if kind is None else kind.ctypes.data,
                                                C.byref(n) if want_count else None), "tsdf_scan_project_filled")
        return dep, kind, (int(n.value) if want_count else None)


    def mark_ground(self, points, params=None, want_flags=True, want_state=True, want_winner=True, want_counts=True):
        """The ground of a scan [n, 4]: (flags [n] uint8: 0 not ground, 1 ground, 2 no cell; state [n_rings, n_columns] int8: 1
        ground, 0 not, -1 the cell or the one above it is empty; winner [n_rings, n_columns] int32: the cell's point or -1;
        counts [4]: points with a cell, occupied cells, ground cells, ground points), None for what was not asked for."""
        pts = _scan_points(points)
        p = _scan_ground_params(params)
        shape = (max(p.n_rings, 0), max(p.n_columns, 0))
        flags = np.empty(len(pts), np.uint8) if want_flags else None
        state = np.empty(shape, np.int8) if want_state else None
        winner = np.empty(shape, np.int32) if want_winner else None
        counts = np.full(4, -1, np.int64) if want_counts else None
        check(self.lib.tsdf_scan_mark_ground(self._h, C.addressof(p), pts.ctypes.data if len(pts) else None, len(pts),
                                             None if flags is None else flags.ctypes.data, None if state is None else state.ctypes.data,
                                             None if winner is None else winner.ctypes.data,
                                             None if counts is None else counts.ctypes.data), "tsdf_scan_mark_ground")
        return flags, state, winner, counts

    def project_ground(self, points, velo2img, K, ground_params=None, select=SCAN_DROP_GROUND, fill_params=None, fill=False,
                       want_range=True, want_depth=True, want_kind=True, want_counts=True):
        """project() -- or, with fill or fill_params, project_filled() -- of the points of a scan that `select` keeps:
        {"range", "depth", "kind" (filled only), "n_pixels", "n_filled" (filled only), "n_selected"}, None for what was not
        asked for."""
        pts = _scan_points(points)
        m, k = _f32(velo2img, 12), _f32(K, 9)
        g = _scan_ground_params(ground_params)
        f = _scan_fill_params(fill_params) if (fill or fill_params is not None) else None
        rng = np.empty((self.h, self.w), np.float32) if want_range else None
        dep = np.empty((self.h, self.w), np.float32) if want_depth else None
        kind = np.empty((self.h, self.w), np.uint8) if (want_kind and f is not None) else None
        n_px, n_fill, n_sel = C.c_int64(-1), C.c_int64(-1), C.c_int64(-1)
        check(self.lib.tsdf_scan_project_ground(self._h, m.ctypes.data, k.ctypes.data, C.addressof(g), int(select),
                                                None if f is None else C.addressof(f), pts.ctypes.data if len(pts) else None, len(pts),
                                                None if rng is None else rng.ctypes.data, None if dep is None else dep.ctypes.data,
                                                None if kind is None else kind.ctypes.data, C.byref(n_px) if want_counts else None,
                                                C.byref(n_fill) if (want_counts and f is not None) else None,
                                                C.byref(n_sel) if want_counts else None), "tsdf_scan_project_ground")
        return {"range": rng, "depth": dep, "kind": kind, "n_pixels": int(n_px.value) if want_counts else None,
                "n_filled": int(n_fill.value) if (want_counts and f is not None) else None,
                "n_selected": int(n_sel.value) if want_counts else None}


def selftest_round(device=0):
    """Returns (mismatches, first_bad[4]) of the exhaustive pixel-rounding self-test."""
    cnt = C.c_uint64()
    bad = (C.c_float * 4)()
    check(load().tsdf_selftest_round(device, C.byref(cnt), bad), "tsdf_selftest_round")
    return cnt.value, list(bad)


def default_brick_shape(cfg):
    """(quads, rows, slices) of the wavefront brick tsdf_create would choose for this grid; host arithmetic only."""
    out = (C.c_int32 * 3)()
    check(load().tsdf_default_brick_shape(C.byref(cfg), out), "tsdf_default_brick_shape")
    return tuple(out)


def selftest_tile_tables(depth_ptr, mask_ptr, im_height, im_width, max_depth=6.0, device=0):
    """Entries of one frame's depth tile table that differ between the launched kernels and the plain ones (must be 0)."""
    cnt = C.c_uint64()
    check(load().tsdf_selftest_tile_tables(device, depth_ptr, mask_ptr, im_height, im_width, max_depth, C.byref(cnt)),
          "tsdf_selftest_tile_tables")
    return cnt.value


class Volume:
    """One z-slab of a TSDF grid in HBM: thin object wrapper over the opaque C handle."""

    def __init__(self, cfg, _borrowed_handle=None):
        self.lib = load()
        self.cfg = cfg
        self._owned = _borrowed_handle is None
        self._h = C.c_void_p()
        if self._owned:
            check(self.lib.tsdf_create(C.byref(cfg), C.byref(self._h)), "tsdf_create")
        else:
            self._h = _borrowed_handle

    # -- lifetime ---------------------------------------------------------------------------
    def close(self):
        if self._h:
            if self._owned:
                self.lib.tsdf_destroy(self._h)
            self._h = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- properties -------------------------------------------------------------------------
    @property
    def n_voxels(self):
        return int(self.lib.tsdf_slab_voxels(self._h))

    def shortcut_stats(self, enable=True):
        """(per-voxel, free-space, skipped) wavefront-frame counts since the counters were enabled; then (re)arm or stop."""
        out = (C.c_uint64 * 3)()
        check(self.lib.tsdf_shortcut_stats(self._h, 1 if enable else 0, out), "tsdf_shortcut_stats")
        return tuple(int(x) for x in out)

    def brick_list_stats(self):
        """(super-bricks every frame skipped, bricks on the work list, of those left to classify themselves, of those skipped
        after all) since shortcut_stats(True)."""
        out = (C.c_uint64 * 4)()
        check(self.lib.tsdf_brick_list_stats(self._h, out), "tsdf_brick_list_stats")
        return tuple(int(x) for x in out)

    def classification_info(self):
        """(fraction of workgroup-frames the last counted launch claimed or -1, launches since one classified)."""
        out = (C.c_double * 2)()
        check(self.lib.tsdf_classification_info(self._h, out), "tsdf_classification_info")
        return float(out[0]), int(out[1])

    def store_stats(self):
        """The handle's slots in the shared staging store: {"frames" | "masks" | "tables": (held, released and not yet reused,
        slots of the class in the store)}.  Applies no collected frame and does not synchronise."""
        out = (C.c_int64 * 9)()
        check(self.lib.tsdf_store_stats(self._h, out), "tsdf_store_stats")
        return {name: tuple(int(x) for x in out[3 * k:3 * k + 3]) for k, name in enumerate(("frames", "masks", "tables"))}

    def summary_stats(self):
        """(segments of the slab, those whose summary word says "every TSDF value is 1", those whose word carries a weight
        run, i.e. "every weight is the count c").  Synchronises the stream."""
        out = (C.c_uint64 * 3)()
        check(self.lib.tsdf_summary_stats(self._h, out), "tsdf_summary_stats")
        return tuple(int(x) for x in out)

    def summary_words(self):
        """The summary words of the slab as a uint32 array, in the kernels' order (include/tsdf_hip_diag.h); empty for a
        grid without summary (dim_x % 4 != 0).  Applies the collected frames and synchronises the stream."""
        n = C.c_int64(0)
        check(self.lib.tsdf_summary_words(self._h, None, 0, C.byref(n)), "tsdf_summary_words")
        out = np.zeros(int(n.value), np.uint32)
        if out.size:
            check(self.lib.tsdf_summary_words(self._h, out.ctypes.data, out.size, C.byref(n)), "tsdf_summary_words")
            assert int(n.value) == out.size
        return out

    @property
    def frames_per_launch(self):
        """Frames a sequence call applies per pass over this slab (1 when the kernel variant does not fuse)."""
        return int(self.lib.tsdf_frames_per_launch(self._h))

    @property
    def slab_shape(self):
        c = self.cfg
        return (c.z_end - c.z_begin, c.dim_y, c.dim_x)

    def device_ptrs(self):
        t, w = C.c_void_p(), C.c_void_p()
        check(self.lib.tsdf_device_ptrs(self._h, C.byref(t), C.byref(w)), "tsdf_device_ptrs")
        return t.value, w.value

    # -- integrate --------------------------------------------------------------------------
    def integrate(self, depth_host, cam2world):
        """TSDF::Integrate semantics: host depth (borrowed for the call), camera pose."""
        d = _f32(depth_host, self.cfg.im_height * self.cfg.im_width)
        p = _f32(cam2world, 16)
        check(self.lib.tsdf_integrate(self._h, d.ctypes.data, p.ctypes.data), "tsdf_integrate")

    def set_deferral(self, n_frames):
        """Host frames collected per launch by integrate() (0 / 1: every call launches; default 32)."""
        check(self.lib.tsdf_set_deferral(self._h, n_frames), "tsdf_set_deferral")

    def integrate_range(self, range_host, cam2world):
        """integrate() for a lidar range image (distance along the ray): converted to z-depth on the device."""
        r = _f32(range_host, self.cfg.im_height * self.cfg.im_width)
        p = _f32(cam2world, 16)
        check(self.lib.tsdf_integrate_range(self._h, r.ctypes.data, p.ctypes.data), "tsdf_integrate_range")

    def integrate_scan(self, points, velo2img, cam2world):
        """integrate() for a lidar scan [n, 4] (x, y, z, intensity): projected on the device, the image never leaves it."""
        pts = _scan_points(points)
        m, p = _f32(velo2img, 12), _f32(cam2world, 16)
        check(self.lib.tsdf_integrate_scan(self._h, m.ctypes.data, pts.ctypes.data if len(pts) else None, len(pts), p.ctypes.data),
              "tsdf_integrate_scan")

    def integrate_range_filled(self, range_host, cam2world, params=None):
        """integrate_range() with the gaps between beams filled on the device (Scanner.fill_depth's rule)."""
        r = _f32(range_host, self.cfg.im_height * self.cfg.im_width)
        p = _f32(cam2world, 16)
        f = _scan_fill_params(params)
        check(self.lib.tsdf_integrate_range_filled(self._h, C.addressof(f), r.ctypes.data, p.ctypes.data), "tsdf_integrate_range_filled")

    def integrate_scan_ground(self, points, velo2img, cam2world, ground_params=None, select=SCAN_DROP_GROUND, fill_params=None,
                              fill=False):
        """integrate_scan() -- or, with fill or fill_params, integrate_scan_filled() -- of the points that `select` keeps
        (Scanner.mark_ground's rule)."""
        pts = _scan_points(points)
        m, p = _f32(velo2img, 12), _f32(cam2world, 16)
        g = _scan_ground_params(ground_params)
        f = _scan_fill_params(fill_params) if (fill or fill_params is not None) else None
        check(self.lib.tsdf_integrate_scan_ground(self._h, m.ctypes.data, C.addressof(g), int(select), None if f is None else C.addressof(f),
                                                  pts.ctypes.data if len(pts) else None, len(pts), p.ctypes.data),
              "tsdf_integrate_scan_ground")

    def integrate_scan_filled(self, points, velo2img, cam2world, params=None):
        """integrate_scan() with the gaps between beams filled on the device (Scanner.fill_depth's rule)."""
        pts = _scan_points(points)
        m, p = _f32(velo2img, 12), _f32(cam2world, 16)
        f = _scan_fill_params(params)
        check(self.lib.tsdf_integrate_scan_filled(self._h, m.ctypes.data, C.addressof(f), pts.ctypes.data if len(pts) else None, len(pts),
                                                  p.ctypes.data), "tsdf_integrate_scan_filled")

    def integrate_u16(self, raw_u16, cam2world, depth_factor=5000.0, row_step=1, col_step=1):
        """Raw 16-bit frame: half-size H2D copy, conversion (and optional subsampling) on the device."""
        r = np.ascontiguousarray(raw_u16, dtype=np.uint16).ravel()
        if r.size != self.cfg.im_height * self.cfg.im_width:
            raise ValueError("raw frame size does not match the configured image")
        p = _f32(cam2world, 16)
        check(self.lib.tsdf_integrate_u16(self._h, r.ctypes.data, depth_factor, row_step, col_step, p.ctypes.data),
              "tsdf_integrate_u16")

    def convert_depth_u16(self, raw_ptr, depth_ptr, depth_factor=5000.0, row_step=1, col_step=1):
        check(self.lib.tsdf_convert_depth_u16(self._h, raw_ptr, depth_ptr, depth_factor, row_step, col_step),
              "tsdf_convert_depth_u16")

    def integrate_device(self, depth_ptr, cam2world):
        p = _f32(cam2world, 16)
        check(self.lib.tsdf_integrate_device(self._h, depth_ptr, p.ctypes.data), "tsdf_integrate_device")

    def integrate_cam2base(self, depth_ptr, cam2base):
        p = _f32(cam2base, 16)
        check(self.lib.tsdf_integrate_cam2base(self._h, depth_ptr, p.ctypes.data), "tsdf_integrate_cam2base")

    def integrate_masked_device(self, depth_ptr, mask_ptr, cam2world):
        p = _f32(cam2world, 16)
        check(self.lib.tsdf_integrate_masked_device(self._h, depth_ptr, mask_ptr, p.ctypes.data),
              "tsdf_integrate_masked_device")

    def integrate_frames_device(self, depth_ptrs, poses, mask_ptrs=None):
        """A known sequence of frames == that many integrate_device calls, possibly fused per launch."""
        p = _f32(np.asarray(poses, dtype=np.float32))
        n = p.size // 16
        assert len(depth_ptrs) == n
        d = (C.c_void_p * n)(*[C.c_void_p(x) for x in depth_ptrs])
        m = None
        if mask_ptrs is not None:
            m = (C.c_void_p * n)(*[C.c_void_p(x) if x else C.c_void_p() for x in mask_ptrs])
        check(self.lib.tsdf_integrate_frames_device(self._h, d, m, p.ctypes.data, n), "tsdf_integrate_frames_device")

    def integrate_sequence_timed(self, depth_ptr, poses):
        """Queue len(poses) frames back to back; returns device milliseconds (HIP events)."""
        p = _f32(np.asarray(poses, dtype=np.float32))
        n = p.size // 16
        ms = C.c_float()
        check(self.lib.tsdf_integrate_sequence_timed(self._h, depth_ptr, p.ctypes.data, n, C.byref(ms)),
              "tsdf_integrate_sequence_timed")
        return ms.value

    def integrate_frames_timed(self, depth_ptrs, poses, mask_ptrs=None):
        """integrate_frames_device bracketed by HIP events on the handle's stream; returns device milliseconds."""
        p = _f32(np.asarray(poses, dtype=np.float32))
        n = p.size // 16
        assert len(depth_ptrs) == n
        d = (C.c_void_p * n)(*[C.c_void_p(x) for x in depth_ptrs])
        m = None
        if mask_ptrs is not None:
            m = (C.c_void_p * n)(*[C.c_void_p(x) if x else C.c_void_p() for x in mask_ptrs])
        ms = C.c_float()
        check(self.lib.tsdf_integrate_frames_timed(self._h, d, m, p.ctypes.data, n, C.byref(ms)),
              "tsdf_integrate_frames_timed")
        return ms.value

    def frames_timed_call(self, depth_ptrs, poses, mask_ptrs=None):
        """integrate_frames_timed with the argument marshalling done ahead of time: returns a callable that queues the
        sequence and returns its device milliseconds (for timed regions that must not include building 10 000 pointers)."""
        p = _f32(np.asarray(poses, dtype=np.float32))
        n = p.size // 16
        assert len(depth_ptrs) == n
        d = (C.c_void_p * n)(*depth_ptrs)
        m = None
        if mask_ptrs is not None:
            m = (C.c_void_p * n)(*[x if x else None for x in mask_ptrs])
        ms = C.c_float()

        def call():
            check(self.lib.tsdf_integrate_frames_timed(self._h, d, m, p.ctypes.data, n, C.byref(ms)), "tsdf_integrate_frames_timed")
            return ms.value
        return call

    def probe_graph_replay(self, depth_ptr, poses, iters=20):
        """(ms per repetition queued call by call, ms per repetition replayed from a captured hipGraph)."""
        p = _f32(np.asarray(poses, dtype=np.float32))
        a, b = C.c_float(), C.c_float()
        check(self.lib.tsdf_probe_graph_replay(self._h, depth_ptr, p.ctypes.data, p.size // 16, iters, C.byref(a), C.byref(b)),
              "tsdf_probe_graph_replay")
        return a.value, b.value

    def probe_stream(self, non_temporal=False, iters=20):
        """Bare RMW stream over the slab (ceiling probe); returns milliseconds per pass."""
        ms = C.c_float()
        check(self.lib.tsdf_probe_stream(self._h, int(non_temporal), iters, C.byref(ms)), "tsdf_probe_stream")
        return ms.value / iters

    def last_cam2base(self):
        out = np.empty(16, np.float32)
        check(self.lib.tsdf_last_cam2base(self._h, out.ctypes.data), "tsdf_last_cam2base")
        return out

    # -- state ------------------------------------------------------------------------------
    def sync(self):
        check(self.lib.tsdf_sync(self._h), "tsdf_sync")

    def reset(self):
        check(self.lib.tsdf_reset(self._h), "tsdf_reset")

    def download(self):
        n = self.n_voxels
        t, w = np.empty(n, np.float32), np.empty(n, np.float32)
        check(self.lib.tsdf_download(self._h, t.ctypes.data, w.ctypes.data), "tsdf_download")
        return t, w

    def copy_slices(self, z_local, n_slices):
        """Host copies of n_slices whole z-slices starting at slab-local z_local."""
        n = n_slices * self.cfg.dim_x * self.cfg.dim_y
        t, w = np.empty(n, np.float32), np.empty(n, np.float32)
        check(self.lib.tsdf_copy_slices(self._h, z_local, n_slices, t.ctypes.data, w.ctypes.data), "tsdf_copy_slices")
        return t, w

    def copy_slices_to_device(self, z_local, n_slices, tsdf_ptr, weight_ptr):
        """Same, into device buffers (e.g. an RCCL send buffer): no host hop."""
        check(self.lib.tsdf_copy_slices(self._h, z_local, n_slices, tsdf_ptr, weight_ptr), "tsdf_copy_slices")

    def upload(self, tsdf, weight):
        t, w = _f32(tsdf, self.n_voxels), _f32(weight, self.n_voxels)
        check(self.lib.tsdf_upload(self._h, t.ctypes.data, w.ctypes.data), "tsdf_upload")

    def set_stream(self, stream_ptr):
        check(self.lib.tsdf_set_stream(self._h, stream_ptr), "tsdf_set_stream")

    def set_kernel_variant(self, v):
        check(self.lib.tsdf_set_kernel_variant(self._h, v), "tsdf_set_kernel_variant")

    def set_brick_shape(self, quads=0, rows=0, slices=0):
        """The box a wavefront owns in classified launches (tuning only; (0, 0, 0) = the library's choice)."""
        check(self.lib.tsdf_set_brick_shape(self._h, quads, rows, slices), "tsdf_set_brick_shape")

    def brick_shape(self):
        out = (C.c_int32 * 3)()
        check(self.lib.tsdf_brick_shape(self._h, out), "tsdf_brick_shape")
        return tuple(out)

    # -- per-voxel label fusion ----------------------------------------------------------------
    def labels_enable(self, prob_threshold=0.5):
        check(self.lib.tsdf_labels_enable(self._h, prob_threshold), "tsdf_labels_enable")

    def compose_labels(self, masks_ptr, labels, scores, label_im_ptr, score_im_ptr):
        lab = np.ascontiguousarray(labels, np.uint16)
        sc = _f32(scores)
        check(self.lib.tsdf_compose_labels(self._h, masks_ptr, lab.ctypes.data, sc.ctypes.data, lab.size,
                                           label_im_ptr, score_im_ptr), "tsdf_compose_labels")

    def integrate_labels_device(self, depth_ptr, label_im_ptr, score_im_ptr, cam2world):
        p = _f32(cam2world, 16)
        check(self.lib.tsdf_integrate_labels_device(self._h, depth_ptr, label_im_ptr, score_im_ptr, p.ctypes.data),
              "tsdf_integrate_labels_device")

    def integrate_frames_labels_device(self, depth_ptrs, label_im_ptrs, score_im_ptrs, poses):
        """Integrate + label fusion of a known sequence in the same passes == integrate_device + integrate_labels_device
        per frame."""
        p = _f32(np.asarray(poses, dtype=np.float32))
        n = p.size // 16
        assert len(depth_ptrs) == len(label_im_ptrs) == len(score_im_ptrs) == n
        arr = lambda xs: (C.c_void_p * n)(*[C.c_void_p(x) for x in xs])
        check(self.lib.tsdf_integrate_frames_labels_device(self._h, arr(depth_ptrs), arr(label_im_ptrs), arr(score_im_ptrs),
                                                           p.ctypes.data, n), "tsdf_integrate_frames_labels_device")

    def download_labels(self):
        n = self.n_voxels
        lab, fp, bp = np.empty(n, np.uint16), np.empty(n, np.float32), np.empty(n, np.float32)
        check(self.lib.tsdf_download_labels(self._h, lab.ctypes.data, fp.ctypes.data, bp.ctypes.data), "tsdf_download_labels")
        return lab, fp, bp

    def upload_labels(self, label, fp, bp):
        n = self.n_voxels
        lab = np.ascontiguousarray(label, np.uint16).ravel()
        if lab.size != n:
            raise ValueError(f"expected {n} labels, got {lab.size}")
        f, b = _f32(fp, n), _f32(bp, n)
        check(self.lib.tsdf_upload_labels(self._h, lab.ctypes.data, f.ctypes.data, b.ctypes.data), "tsdf_upload_labels")

    # -- per-voxel colour fusion ----------------------------------------------------------------
    def colour_enable(self):
        check(self.lib.tsdf_colour_enable(self._h), "tsdf_colour_enable")

    def integrate_colour_device(self, depth_ptr, rgb_ptr, cam2world):
        """Colour pass of the frame just integrated (queue right after integrate*_device of the same frame)."""
        p = _f32(cam2world, 16)
        check(self.lib.tsdf_integrate_colour_device(self._h, depth_ptr, rgb_ptr, p.ctypes.data), "tsdf_integrate_colour_device")

    def integrate_rgbd(self, depth_host, rgb_host, cam2world):
        d = _f32(depth_host, self.cfg.im_height * self.cfg.im_width)
        c = np.ascontiguousarray(rgb_host, dtype=np.uint8).ravel()
        if c.size != 3 * self.cfg.im_height * self.cfg.im_width:
            raise ValueError("colour image must be height x width x 3 bytes")
        p = _f32(cam2world, 16)
        check(self.lib.tsdf_integrate_rgbd(self._h, d.ctypes.data, c.ctypes.data, p.ctypes.data), "tsdf_integrate_rgbd")

    def download_colour(self):
        out = np.empty(self.n_voxels, np.uint32)
        check(self.lib.tsdf_download_colour(self._h, out.ctypes.data), "tsdf_download_colour")
        return out

    def upload_colour(self, colour):
        c = np.ascontiguousarray(colour, np.uint32).ravel()
        if c.size != self.n_voxels:
            raise ValueError(f"expected {self.n_voxels} colours, got {c.size}")
        check(self.lib.tsdf_upload_colour(self._h, c.ctypes.data), "tsdf_upload_colour")

    # -- raycasting -------------------------------------------------------------------------
    def raycast(self, cam2world, params=None, normals=True, labels=False, colour=False):
        """Render the volume from cam2world (csrc/tsdf_raycast.hip.h): dict of host arrays "depth" [H, W] float32 and, as
        asked, "normal" [H, W, 3] float32 (camera frame), "label" [H, W] uint16, "colour" [H, W] uint32.  params: a
        RaycastParams, default raycast_params_default(cfg)."""
        p = raycast_params_default(self.cfg) if params is None else params
        h, w = p.im_height, p.im_width
        out = {"depth": np.empty((h, w), np.float32)}
        if normals:
            out["normal"] = np.empty((h, w, 3), np.float32)
        if labels:
            out["label"] = np.empty((h, w), np.uint16)
        if colour:
            out["colour"] = np.empty((h, w), np.uint32)
        ptr = lambda k: out[k].ctypes.data if k in out else None
        c2w = _f32(cam2world, 16)
        check(self.lib.tsdf_raycast(self._h, C.byref(p), c2w.ctypes.data, ptr("depth"), ptr("normal"), ptr("label"),
                                    ptr("colour")), "tsdf_raycast")
        return out

    def raycast_device(self, cam2world, depth_ptr, normal_ptr=None, label_ptr=None, colour_ptr=None, params=None):
        """The same into device buffers (pointers, each may be None), queued on the handle's stream."""
        p = raycast_params_default(self.cfg) if params is None else params
        c2w = _f32(cam2world, 16)
        check(self.lib.tsdf_raycast_device(self._h, C.byref(p), c2w.ctypes.data, depth_ptr, normal_ptr, label_ptr, colour_ptr),
              "tsdf_raycast_device")

    def track(self, depth_ptr, guess_cam2world, params=None, mask_ptr=None):
        """Track a live depth frame (device pointer, params.ray's image size) against the model from guess_cam2world
        (csrc/tsdf_track.hip.h).  Returns (cam2world [4, 4] float32, stats dict with status, status_name, iters_run,
        inliers, rmse); a lost track returns the guess itself with status 2.  params: a TrackParams, default
        track_params_default(cfg)."""
        p = track_params_default(self.cfg) if params is None else params
        guess = _f32(guess_cam2world, 16)
        res = TrackResult()
        check(self.lib.tsdf_track(self._h, C.byref(p), depth_ptr, mask_ptr, guess.ctypes.data, C.byref(res)), "tsdf_track")
        pose = np.array(res.cam2world, np.float32).reshape(4, 4)
        stats = {"status": res.status, "status_name": TRACK_STATUS[res.status], "iters_run": list(res.iters_run),
                 "inliers": res.inliers, "rmse": res.rmse}
        return pose, stats

    def track_system(self, depth_ptr, ref_cam2world, cam2world, level=0, params=None, mask_ptr=None):
        """The linear system of one iteration at `level`, model rendered at ref_cam2world, pairs at cam2world:
        (A = J^T J [6, 6] float64, b = J^T r [6], sum r^2, pair count)."""
        p = track_params_default(self.cfg) if params is None else params
        ref, cur = _f32(ref_cam2world, 16), _f32(cam2world, 16)
        out = np.zeros(29, np.float64)
        check(self.lib.tsdf_track_system(self._h, C.byref(p), depth_ptr, mask_ptr, ref.ctypes.data, cur.ctypes.data, level,
                                         out.ctypes.data), "tsdf_track_system")
        A = np.zeros((6, 6))
        A[np.triu_indices(6)] = out[:21]
        A = A + np.triu(A, 1).T
        return A, out[21:27].copy(), float(out[27]), int(out[28])

    def _host_frame(self, p, depth, rgb, mask):
        """The host images of a photometric call as contiguous arrays of params.ray's size (rgb and mask may be None)."""
        hw = (p.ray.im_height, p.ray.im_width)
        d = np.ascontiguousarray(depth, np.float32)
        c = None if rgb is None else np.ascontiguousarray(rgb, np.uint8)
        m = None if mask is None else np.ascontiguousarray(mask, np.uint8)
        if d.shape != hw or (c is not None and c.shape != hw + (3,)) or (m is not None and m.shape != hw):
            raise ValueError(f"expected images of {hw[0]} x {hw[1]} pixels")
        return d, c, m

    def track_rgbd(self, depth, rgb, guess_cam2world, params=None, photo=None, mask=None):
        """Track a live RGB-D frame (host arrays: depth [H, W] float32, rgb [H, W, 3] uint8 or None, mask [H, W] uint8 or
        None) against the model from guess_cam2world with the geometric and the photometric term (csrc/tsdf_photo.hip.h).
        Returns (cam2world [4, 4] float32, stats as track's plus photo_pairs, photo_rmse).  photo: a PhotoParams, default
        photo_params_default(cfg); rgb None or photo_weight 0 is the geometric track."""
        p = track_params_default(self.cfg) if params is None else params
        pp = photo_params_default(self.cfg) if photo is None else photo
        d, c, m = self._host_frame(p, depth, rgb, mask)
        guess = _f32(guess_cam2world, 16)
        res = TrackRgbdResult()
        check(self.lib.tsdf_track_rgbd(self._h, C.byref(p), C.byref(pp), d.ctypes.data, None if c is None else c.ctypes.data,
                                       None if m is None else m.ctypes.data, guess.ctypes.data, C.byref(res)), "tsdf_track_rgbd")
        g = res.geo
        pose = np.array(g.cam2world, np.float32).reshape(4, 4)
        stats = {"status": g.status, "status_name": TRACK_STATUS[g.status], "iters_run": list(g.iters_run),
                 "inliers": g.inliers, "rmse": g.rmse, "photo_pairs": res.photo_pairs, "photo_rmse": res.photo_rmse}
        return pose, stats

    def track_rgbd_system(self, depth, rgb, ref_cam2world, cam2world, level=0, params=None, photo=None, mask=None):
        """Both systems of one iteration at `level` (tsdf_track_rgbd_system): (geo [29], photo [29]) float64 in
        tsdf_track_system's layout, unweighted."""
        p = track_params_default(self.cfg) if params is None else params
        pp = photo_params_default(self.cfg) if photo is None else photo
        d, c, m = self._host_frame(p, depth, rgb, mask)
        ref, cur = _f32(ref_cam2world, 16), _f32(cam2world, 16)
        geo, pho = np.zeros(29, np.float64), np.zeros(29, np.float64)
        check(self.lib.tsdf_track_rgbd_system(self._h, C.byref(p), C.byref(pp), d.ctypes.data,
                                              None if c is None else c.ctypes.data, None if m is None else m.ctypes.data,
                                              ref.ctypes.data, cur.ctypes.data, level, geo.ctypes.data, pho.ctypes.data),
              "tsdf_track_rgbd_system")
        return geo, pho

    def render_intensity(self, cam2world, level=0, params=None):
        """The model intensity image of pyramid level `level` from cam2world (tsdf_render_intensity): float32
        [H >> level, W >> level], -1 where the model has none.  params: a RaycastParams."""
        p = raycast_params_default(self.cfg) if params is None else params
        out = np.empty((p.im_height >> max(level, 0), p.im_width >> max(level, 0)), np.float32)
        c2w = _f32(cam2world, 16)
        check(self.lib.tsdf_render_intensity(self._h, C.byref(p), c2w.ctypes.data, level, out.ctypes.data),
              "tsdf_render_intensity")
        return out

    # -- merging ----------------------------------------------------------------------------
    def fuse_from(self, src, params=None, dst2src=None, carry=0):
        """Merge the volume `src` into this one by trilinear resampling (csrc/tsdf_fuse.hip.h): every voxel of this grid
        samples src at its own position.  params: a FuseParams, default fuse_params_default(cfg); write = 0 compares only.
        dst2src: the pose to sample through (16 float32, this grid's base frame to src's; tsdf_fuse_volume_at) in place of
        the one the two base2world give.  Returns the counts as a dict: sampled, both, both_band, agree_band.
        carry: FUSE_CARRY_COLOUR | FUSE_CARRY_LABELS -- the updated voxels also take src's colour and / or label evidence
        (tsdf_fuse_volume_carry, csrc/tsdf_fuse_carry.hip.h); the dict then also holds label_adopted, label_agreed,
        label_opposed and label_flipped."""
        p = fuse_params_default(self.cfg) if params is None else params
        c = FuseCounts()
        if carry:
            m = None if dst2src is None else _f32(dst2src, 16)
            cc = FuseCarryCounts()
            check(self.lib.tsdf_fuse_volume_carry(self._h, src._h, C.byref(p), None if m is None else m.ctypes.data, carry,
                                                  C.byref(c), C.byref(cc)), "tsdf_fuse_volume_carry")
            return {"sampled": int(c.sampled), "both": int(c.both), "both_band": int(c.both_band),
                    "agree_band": int(c.agree_band), "label_adopted": int(cc.label_adopted),
                    "label_agreed": int(cc.label_agreed), "label_opposed": int(cc.label_opposed),
                    "label_flipped": int(cc.label_flipped)}
        if dst2src is None:
            check(self.lib.tsdf_fuse_volume(self._h, src._h, C.byref(p), C.byref(c)), "tsdf_fuse_volume")
        else:
            m = _f32(dst2src, 16)
            check(self.lib.tsdf_fuse_volume_at(self._h, src._h, C.byref(p), m.ctypes.data, C.byref(c)), "tsdf_fuse_volume_at")
        return {"sampled": int(c.sampled), "both": int(c.both), "both_band": int(c.both_band),
                "agree_band": int(c.agree_band)}

    # -- registration -----------------------------------------------------------------------
    def align_to(self, src, params=None, guess=None):
        """Register this volume (the destination) against `src` (csrc/tsdf_align.hip.h).  Returns (dst2src [4, 4] float32,
        status dict with status, status_name, iters_run, pairs, rmse); a lost run returns the start itself with status 2.
        params: an AlignParams, default align_params_default(cfg); guess: the starting dst2src (16 float32), default the
        pose the two base2world give (fuse_pose_default).  Reads both volumes only."""
        p = align_params_default(self.cfg) if params is None else params
        g = None if guess is None else _f32(guess, 16)
        res = AlignResult()
        check(self.lib.tsdf_align_volume(self._h, src._h, C.byref(p), None if g is None else g.ctypes.data, C.byref(res)),
              "tsdf_align_volume")
        pose = np.array(res.dst2src, np.float32).reshape(4, 4)
        return pose, {"status": res.status, "status_name": TRACK_STATUS[res.status], "iters_run": list(res.iters_run),
                      "pairs": res.pairs, "rmse": res.rmse}

    def align_system(self, src, dst2src, level=0, params=None):
        """The linear system of one registration pass at `level` and the pose dst2src: (A = J^T J [6, 6] float64,
        b = J^T r [6], sum r^2, pair count)."""
        p = align_params_default(self.cfg) if params is None else params
        m = _f32(dst2src, 16)
        out = np.zeros(29, np.float64)
        check(self.lib.tsdf_align_system(self._h, src._h, C.byref(p), m.ctypes.data, level, out.ctypes.data), "tsdf_align_system")
        A = np.zeros((6, 6))
        A[np.triu_indices(6)] = out[:21]
        A = A + np.triu(A, 1).T
        return A, out[21:27].copy(), float(out[27]), int(out[28])

    # -- tracking a lidar scan --------------------------------------------------------------
    def track_scan(self, points, guess_velo2world, params=None, flags=None):
        """Track a lidar scan [n, 4] against this volume, point to signed distance (csrc/tsdf_scan_track.hip.h).  Returns
        (velo2world [4, 4] float32, status dict with status, status_name, iters_run, pairs, rmse); a lost run returns the
        guess itself with status 2.  params: a ScanTrackParams, default scan_track_params_default(cfg); flags: n bytes
        (Scanner.mark_ground's), looked at when params.drop_flag >= 0.  Reads the volume only."""
        p = scan_track_params_default(self.cfg) if params is None else params
        pts = _scan_points(points)
        f = _scan_flags(flags, len(pts))
        g = _f32(guess_velo2world, 16)
        res = ScanTrackResult()
        check(self.lib.tsdf_scan_track(self._h, C.byref(p), pts.ctypes.data if len(pts) else None, len(pts),
                                       None if f is None or not len(pts) else f.ctypes.data, g.ctypes.data, C.byref(res)), "tsdf_scan_track")
        pose = np.array(res.velo2world, np.float32).reshape(4, 4)
        return pose, {"status": res.status, "status_name": TRACK_STATUS[res.status], "iters_run": list(res.iters_run),
                      "pairs": res.pairs, "rmse": res.rmse}

    def track_scan_system(self, points, velo2world, level=0, params=None, flags=None):
        """The 29 sums of one scan tracking pass at `level` and the pose velo2world (tsdf_scan_track_system): 21 of J^T J (upper
        triangle), 6 of J^T r, sum r^2, the pair count; float64 [29]."""
        p = scan_track_params_default(self.cfg) if params is None else params
        pts = _scan_points(points)
        f = _scan_flags(flags, len(pts))
        m = _f32(velo2world, 16)
        out = np.zeros(29, np.float64)
        check(self.lib.tsdf_scan_track_system(self._h, C.byref(p), pts.ctypes.data if len(pts) else None, len(pts),
                                              None if f is None or not len(pts) else f.ctypes.data, m.ctypes.data, level, out.ctypes.data),
              "tsdf_scan_track_system")
        return out

    # -- extent -----------------------------------------------------------------------------
    def extent(self, params=None):
        """What the slab holds (csrc/tsdf_extent.hip.h): an Extent record -- observed and near-surface voxel counts, sums,
        second moments, index bounds (GLOBAL z) and border counts.  params: an ExtentParams, default
        extent_params_default(cfg).  Reads the volume only."""
        p = extent_params_default(self.cfg) if params is None else params
        e = Extent()
        check(self.lib.tsdf_volume_extent(self._h, C.byref(p), C.byref(e)), "tsdf_volume_extent")
        return e

    # -- outputs ----------------------------------------------------------------------------
    def count_surface(self, weight_thresh=0.9):
        n = C.c_int64()
        check(self.lib.tsdf_count_surface(self._h, weight_thresh, C.byref(n)), "tsdf_count_surface")
        return n.value

    def extract_surface(self, weight_thresh=0.9):
        n = self.count_surface(weight_thresh)
        xyz = np.empty((n, 3), np.float32)
        got = C.c_int64()
        check(self.lib.tsdf_extract_surface(self._h, weight_thresh, xyz.ctypes.data, n, C.byref(got)),
              "tsdf_extract_surface")
        assert got.value == n
        return xyz

    def extract_crossings(self, halo=None, weight_thresh=0.9):
        """Zero-crossing vertices of the slab; halo = (tsdf, weight) of slice z_end as numpy arrays,
        or a pair of device pointers (ints), or None on the top slab."""
        ht = hw = None
        keep = None
        if halo is not None:
            if isinstance(halo[0], (int, np.integer)):
                ht, hw = int(halo[0]), int(halo[1])
            else:
                keep = (_f32(halo[0]), _f32(halo[1]))
                ht, hw = keep[0].ctypes.data, keep[1].ctypes.data
        n = C.c_int64()
        check(self.lib.tsdf_extract_crossings(self._h, ht, hw, weight_thresh, None, 0, C.byref(n)), "tsdf_extract_crossings")
        xyz = np.empty((n.value, 3), np.float32)
        if n.value:
            got = C.c_int64()
            check(self.lib.tsdf_extract_crossings(self._h, ht, hw, weight_thresh, xyz.ctypes.data, n.value, C.byref(got)),
                  "tsdf_extract_crossings")
            assert got.value == n.value
        return xyz

    def extract_mesh(self, halo=None, weight_thresh=0.9):
        """Marching-tetrahedra triangles of the slab, array [n, 3, 3]; halo as for extract_crossings."""
        ht = hw = None
        keep = None
        if halo is not None:
            if isinstance(halo[0], (int, np.integer)):
                ht, hw = int(halo[0]), int(halo[1])
            else:
                keep = (_f32(halo[0]), _f32(halo[1]))
                ht, hw = keep[0].ctypes.data, keep[1].ctypes.data
        n = C.c_int64()
        check(self.lib.tsdf_extract_mesh(self._h, ht, hw, weight_thresh, None, 0, C.byref(n)), "tsdf_extract_mesh")
        tri = np.empty((n.value, 3, 3), np.float32)
        if n.value:
            got = C.c_int64()
            check(self.lib.tsdf_extract_mesh(self._h, ht, hw, weight_thresh, tri.ctypes.data, n.value, C.byref(got)),
                  "tsdf_extract_mesh")
            assert got.value == n.value
        return tri

    def save_mesh_ply(self, path, weight_thresh=0.9):
        check(self.lib.tsdf_save_mesh_ply(self._h, os.fsencode(path), weight_thresh), "tsdf_save_mesh_ply")

    def save_mesh_welded_ply(self, path, weight_thresh=0.9):
        check(self.lib.tsdf_save_mesh_welded_ply(self._h, os.fsencode(path), weight_thresh), "tsdf_save_mesh_welded_ply")

    def save_ply(self, path, weight_thresh=0.9):
        check(self.lib.tsdf_save_ply(self._h, os.fsencode(path), weight_thresh), "tsdf_save_ply")

    def save_bin(self, path):
        check(self.lib.tsdf_save_bin(self._h, os.fsencode(path)), "tsdf_save_bin")

    def load_bin(self, path):
        check(self.lib.tsdf_load_bin(self._h, os.fsencode(path)), "tsdf_load_bin")

    def save_state(self, path):
        check(self.lib.tsdf_save_state(self._h, os.fsencode(path)), "tsdf_save_state")

    def load_state(self, path):
        check(self.lib.tsdf_load_state(self._h, os.fsencode(path)), "tsdf_load_state")


class Batch:
    """n per-object volumes integrated by one launch per frame (tsdf_batch_*)."""

    def __init__(self, cfgs):
        self.lib = load()
        self.cfgs = list(cfgs)
        arr = (TsdfConfig * len(self.cfgs))(*self.cfgs)
        self._h = C.c_void_p()
        check(self.lib.tsdf_batch_create(arr, len(self.cfgs), C.byref(self._h)), "tsdf_batch_create")
        self.volumes = []
        for i, cfg in enumerate(self.cfgs):
            h = C.c_void_p()
            check(self.lib.tsdf_batch_volume(self._h, i, C.byref(h)), "tsdf_batch_volume")
            self.volumes.append(Volume(cfg, _borrowed_handle=h))

    def integrate_device(self, depth_ptr, mask_ptrs, cam2world):
        """mask_ptrs: list of device pointers (or None entries), or None for no masks at all."""
        p = _f32(cam2world, 16)
        masks = None
        if mask_ptrs is not None:
            masks = (C.c_void_p * len(self.cfgs))(*[C.c_void_p(m) if m else C.c_void_p() for m in mask_ptrs])
        check(self.lib.tsdf_batch_integrate_device(self._h, depth_ptr, masks, p.ctypes.data), "tsdf_batch_integrate_device")

    def sync(self):
        check(self.lib.tsdf_batch_sync(self._h), "tsdf_batch_sync")

    def raycast_device(self, cam2world, depth_ptr, normal_ptr=None, member_ptr=None, params=None):
        """Every member into one image (nearest hit wins, ties to the lower index; member -1 = miss), device pointers (each
        may be None), queued on the batch's stream.  params default: raycast_params_default of the first member's config."""
        p = raycast_params_default(self.cfgs[0]) if params is None else params
        c2w = _f32(cam2world, 16)
        check(self.lib.tsdf_batch_raycast_device(self._h, C.byref(p), c2w.ctypes.data, depth_ptr, normal_ptr, member_ptr),
              "tsdf_batch_raycast_device")

    def associate(self, cam2world, depth_ptr, masks_ptr, k, params=None, labels=None):
        """Which member each of the k instance masks (masks_ptr: k contiguous H x W byte images on the device) shows in the
        live frame depth_ptr at cam2world (tsdf_batch_associate).  params default: associate_params_default of the first
        member's config; labels: None or (mask_label, mask_score, member_label, member_score).  Returns a dict: overlap
        [k, M, 3], mask [k, 3], member [M, 4] (views of the count block `counts`), assign int32 [k] (-1: no member),
        iou float32 [k]."""
        p = associate_params_default(self.cfgs[0]) if params is None else params
        c2w = _f32(cam2world, 16)
        n = len(self.cfgs)
        counts = np.empty(3 * k * n + 3 * k + 4 * n, np.uint32)
        assign, iou = np.empty(k, np.int32), np.empty(k, np.float32)
        lab, keep = _associate_labels(labels)
        check(self.lib.tsdf_batch_associate(self._h, C.byref(p), c2w.ctypes.data, depth_ptr, masks_ptr, k, lab,
                                            counts.ctypes.data, assign.ctypes.data, iou.ctypes.data), "tsdf_batch_associate")
        del keep
        overlap, mask, member = associate_split(counts, k, n)
        return {"counts": counts, "overlap": overlap, "mask": mask, "member": member, "assign": assign, "iou": iou}

    def track(self, depth_ptr, guess_cam2world, params=None, mask_ptr=None, use=None, want_systems=True):
        """Track a live depth frame (device pointer) against all members together from guess_cam2world
        (csrc/tsdf_batch_track.hip.h).  use: None (all) or one flag per member, nonzero = the member's pairs enter the joint
        system.  Returns (cam2world [4, 4] float32, stats as Volume.track's, systems): systems is float64 [M, 29], every
        member's own system at the final estimate (used or not; all zero on a lost track), or None without want_systems.
        params default: track_params_default of the first member's config."""
        p = track_params_default(self.cfgs[0]) if params is None else params
        guess = _f32(guess_cam2world, 16)
        n = len(self.cfgs)
        flags = None
        if use is not None:
            flags = np.ascontiguousarray(np.asarray(use) != 0, np.uint8)
            if flags.shape != (n,):
                raise ValueError(f"use has {flags.size} flags, the batch {n} members")
        systems = np.zeros((n, 29), np.float64) if want_systems else None
        res = TrackResult()
        check(self.lib.tsdf_batch_track(self._h, C.byref(p), depth_ptr, mask_ptr, None if flags is None else flags.ctypes.data,
                                        guess.ctypes.data, C.byref(res), None if systems is None else systems.ctypes.data),
              "tsdf_batch_track")
        pose = np.array(res.cam2world, np.float32).reshape(4, 4)
        stats = {"status": res.status, "status_name": TRACK_STATUS[res.status], "iters_run": list(res.iters_run),
                 "inliers": res.inliers, "rmse": res.rmse}
        return pose, stats, systems

    def track_system(self, depth_ptr, ref_cam2world, cam2world, level=0, params=None, mask_ptr=None):
        """Every member's system of one pass at `level`, the model rendered at ref_cam2world, the pairs at cam2world:
        float64 [M, 29] in tsdf_track_system's layout (tsdf_batch_track_system)."""
        p = track_params_default(self.cfgs[0]) if params is None else params
        ref, cur = _f32(ref_cam2world, 16), _f32(cam2world, 16)
        out = np.zeros((len(self.cfgs), 29), np.float64)
        check(self.lib.tsdf_batch_track_system(self._h, C.byref(p), depth_ptr, mask_ptr, ref.ctypes.data, cur.ctypes.data,
                                               level, out.ctypes.data), "tsdf_batch_track_system")
        return out

    def extents(self, params=None):
        """The Extent record of every member, by one launch (tsdf_batch_extents).  params default: extent_params_default of
        the first member's config."""
        p = extent_params_default(self.cfgs[0]) if params is None else params
        arr = (Extent * len(self.cfgs))()
        check(self.lib.tsdf_batch_extents(self._h, C.byref(p), arr), "tsdf_batch_extents")
        return list(arr)

    def close(self):
        if self._h:
            for v in self.volumes:
                v.close()
            self.lib.tsdf_batch_destroy(self._h)
            self._h = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


class Group:
    """One grid cut into z-slabs over several devices in one process (tsdf_group_*)."""

    def __init__(self, cfg, devices):
        self.lib = load()
        self.cfg = cfg
        self.devices = [int(d) for d in devices]
        arr = (C.c_int32 * len(self.devices))(*self.devices)
        self._h = C.c_void_p()
        check(self.lib.tsdf_group_create(C.byref(cfg), arr, len(self.devices), C.byref(self._h)), "tsdf_group_create")
        self.slabs = []
        for i in range(len(self.devices)):
            h = C.c_void_p()
            check(self.lib.tsdf_group_volume(self._h, i, C.byref(h)), "tsdf_group_volume")
            c = TsdfConfig()
            check(self.lib.tsdf_get_config(h, C.byref(c)), "tsdf_get_config")
            self.slabs.append(Volume(c, _borrowed_handle=h))

    @property
    def n_voxels(self):
        return int(self.lib.tsdf_group_voxels(self._h))

    def integrate(self, depth_host, cam2world):
        d = _f32(depth_host, self.cfg.im_height * self.cfg.im_width)
        p = _f32(cam2world, 16)
        check(self.lib.tsdf_group_integrate(self._h, d.ctypes.data, p.ctypes.data), "tsdf_group_integrate")

    def integrate_frames(self, depths_host, poses):
        keep = [_f32(d, self.cfg.im_height * self.cfg.im_width) for d in depths_host]
        p = _f32(np.asarray(poses, dtype=np.float32))
        n = p.size // 16
        assert len(keep) == n
        ptrs = (C.c_void_p * n)(*[C.c_void_p(d.ctypes.data) for d in keep])
        check(self.lib.tsdf_group_integrate_frames(self._h, ptrs, p.ctypes.data, n), "tsdf_group_integrate_frames")

    def set_deferral(self, n_frames):
        check(self.lib.tsdf_group_set_deferral(self._h, n_frames), "tsdf_group_set_deferral")

    def sync(self):
        check(self.lib.tsdf_group_sync(self._h), "tsdf_group_sync")

    def reset(self):
        check(self.lib.tsdf_group_reset(self._h), "tsdf_group_reset")

    def download(self):
        n = self.n_voxels
        t, w = np.empty(n, np.float32), np.empty(n, np.float32)
        check(self.lib.tsdf_group_download(self._h, t.ctypes.data, w.ctypes.data), "tsdf_group_download")
        return t, w

    def _list(self, fn, shape, weight_thresh):
        n = C.c_int64()
        check(fn(self._h, weight_thresh, None, 0, C.byref(n)), "tsdf_group_extract")
        out = np.empty((n.value,) + shape, np.float32)
        if n.value:
            got = C.c_int64()
            check(fn(self._h, weight_thresh, out.ctypes.data, n.value, C.byref(got)), "tsdf_group_extract")
            assert got.value == n.value
        return out

    def extract_surface(self, weight_thresh=0.9):
        return self._list(self.lib.tsdf_group_extract_surface, (3,), weight_thresh)

    def extract_crossings(self, weight_thresh=0.9):
        return self._list(self.lib.tsdf_group_extract_crossings, (3,), weight_thresh)

    def extract_mesh(self, weight_thresh=0.9):
        return self._list(self.lib.tsdf_group_extract_mesh, (3, 3), weight_thresh)

    def save_ply(self, path, weight_thresh=0.9):
        check(self.lib.tsdf_group_save_ply(self._h, os.fsencode(path), weight_thresh), "tsdf_group_save_ply")

    def save_mesh_ply(self, path, weight_thresh=0.9):
        check(self.lib.tsdf_group_save_mesh_ply(self._h, os.fsencode(path), weight_thresh), "tsdf_group_save_mesh_ply")

    def save_bin(self, path):
        check(self.lib.tsdf_group_save_bin(self._h, os.fsencode(path)), "tsdf_group_save_bin")

    def extent(self, params=None):
        """The Extent record of the whole grid: every slab's, combined (tsdf_group_extent)."""
        p = extent_params_default(self.cfg) if params is None else params
        e = Extent()
        check(self.lib.tsdf_group_extent(self._h, C.byref(p), C.byref(e)), "tsdf_group_extent")
        return e

    def close(self):
        if self._h:
            for v in self.slabs:
                v.close()
            self.lib.tsdf_group_destroy(self._h)
            self._h = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
