"""ctypes binding of libvistaf_ftp.so (the C ABI declared in include/vistaf_ftp.h).

There is no CPU fallback: if the HIP library is missing or does not load, importing the product
API raises immediately.
"""
from __future__ import annotations

import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libvistaf_ftp.so")

NSCALARS = 16
NREFINFO = 8
NCONTACT = 16           # doubles per row of the per-contact table (VISTAF_NCONTACT)
MAX_CONTACTS = 64
NTRACK = 16             # doubles per row of the contact tracker's table (VISTAF_NTRACK, include/vistaf_track.h)
# fields of a row in the order of the VISTAF_TRACK_* indices; 10..15 are reserved
TRACK_NAMES = ["track_id", "age_frames", "parent_row", "events", "overlap_px", "dx", "dy", "dforce_N", "dvolume_cm3", "origin_track_id"]
TRACK_EVENTS = {"born": 1, "split": 2, "merged": 4, "gated": 8}       # VISTAF_TRACKEV_*, bits of the `events` field
FATE_ENDED, FATE_NO_ROW = -1, -2 ** 31                              # d_fate codes; -(2 + j): absorbed into contact j; >= 0: the continuing row
NSHAPE = 24             # doubles per row of the per-contact shape table (VISTAF_NSHAPE, include/vistaf_shape.h)
# fields of a row in the order of the VISTAF_SHAPE_* indices; 18..23 are reserved
SHAPE_NAMES = ["contact_pixels", "boundary_pixels", "footprint_cx", "footprint_cy", "major_axis_mm", "minor_axis_mm", "orientation_rad",
               "fit_pixels", "fit_status", "apex_x", "apex_y", "apex_depth_mm", "curvature_1_per_mm", "curvature_2_per_mm",
               "curvature_axis_rad", "radius_1_mm", "radius_2_mm", "fit_rms_mm"]
SHAPE_FIT = {"ok": 0, "none": 1, "not_a_cap": 2}                     # VISTAF_SHAPEFIT_*, values of the `fit_status` field
NTAXEL, NTAXELFRAME, TAXEL_NONE = 12, 8, 0xFFFF                      # VISTAF_NTAXEL, VISTAF_NTAXELFRAME, VISTAF_TAXEL_NONE (include/vistaf_taxel.h)
# fields of a taxel row in the order of the VISTAF_TAXEL_* indices (10, 11 are reserved), and of a frame row (VISTAF_TAXELFRAME_*)
TAXEL_NAMES = ["contact_pixels", "contact_area_mm2", "volume_cm3", "mean_depth_mm", "max_depth_mm", "argmax_index", "centroid_x", "centroid_y",
               "force_N", "pressure_kPa"]
TAXEL_FRAME_NAMES = ["active_taxels", "volume_cm3", "force_N", "cop_x", "cop_y", "moment_x_Nmm", "moment_y_Nmm", "peak_taxel"]
NTHERMAL, NTHERMALFRAME = 16, 8                                      # VISTAF_NTHERMAL, VISTAF_NTHERMALFRAME (include/vistaf_thermal.h)
# fields of a thermal row in the order of the VISTAF_THERMAL_* indices (12..15 are reserved), and of a frame row (VISTAF_THERMALFRAME_*; 7 is reserved)
THERMAL_NAMES = ["contact_pixels", "valid_pixels", "coverage", "mean_C", "weighted_mean_C", "min_C", "max_C", "std_C", "peak_temp_C",
                 "surround_pixels", "surround_mean_C", "contrast_C"]
THERMAL_FRAME_NAMES = ["registered_pixels", "skin_mean_C", "contact_pixels", "contact_mean_C", "contrast_C", "hottest_contact", "coldest_contact"]
NTEMPORAL = 16          # doubles per frame row of the temporal read-out (VISTAF_NTEMPORAL, include/vistaf_temporal.h)
# fields of a frame row in the order of the VISTAF_TEMPORAL_* indices
TEMPORAL_NAMES = ["touch_pixels", "onset_pixels", "release_pixels", "loading_pixels", "unloading_pixels", "filtered_volume_cm3", "dvolume_cm3_per_s",
                  "max_filtered_mm", "argmax_index", "max_rate_mm_per_s", "max_rate_index", "min_rate_mm_per_s", "min_rate_index",
                  "longest_dwell_frames", "events", "gap_frames"]
TEMPORAL_EVENTS = {"touch_began": 1, "touch_ended": 2}                # VISTAF_TEMPEV_*, bits of the `events` field
NCLOUD_POINT, NCLOUD_FRAME = 8, 12                                   # VISTAF_NCLOUD_POINT, VISTAF_NCLOUD_FRAME (include/vistaf_cloud.h)
# fields of a point record in the order of the VISTAF_CLOUD_* indices, and of a frame row (VISTAF_CLOUDFRAME_*; 11 is reserved)
CLOUD_POINT_NAMES = ["x", "y", "z", "nx", "ny", "nz", "curvature", "gaussian_curvature"]
CLOUD_FRAME_NAMES = ["surface_pixels", "points", "points_written", "projected_area_mm2", "surface_area_mm2", "mean_normal_x", "mean_normal_y",
                     "mean_normal_z", "tilt_deg", "max_slope_deg", "max_slope_index"]
# launch geometry of the point-cloud kernels (VISTAF_CLOUD_CHUNK_THREADS, _SCAN_THREADS, _ROW_LANES, _ROW_UNROLL): fixes the order of the frame sums
CLOUD_CHUNK_THREADS, CLOUD_SCAN_THREADS, CLOUD_ROW_LANES, CLOUD_ROW_UNROLL = 256, 1024, 64, 4
NMOTION, NMOTIONFRAME = 24, 8                                       # VISTAF_NMOTION, VISTAF_NMOTIONFRAME (include/vistaf_motion.h)
# fields of a motion row in the order of the VISTAF_MOTION_* indices (20..23 are reserved), and of a frame row (VISTAF_MOTIONFRAME_*)
MOTION_NAMES = ["parent_row", "template_pixels", "status", "iterations", "tx_px", "ty_px", "theta_rad", "beta_mm", "tx_mm", "ty_mm", "centre_x",
                "centre_y", "rms_before_mm", "rms_after_mm", "last_step_px", "se_tx_px", "se_ty_px", "se_theta_rad", "tx_minus_dx", "ty_minus_dy"]
MOTION_FRAME_NAMES = ["registered", "max_slide_mm", "max_slide_row", "max_twist_rad", "max_twist_row", "mean_tx_mm", "mean_ty_mm", "mean_rms_after_mm"]
MOTION_STATUS = {"ok": 0, "not_converged": 1, "no_parent": 2, "too_few": 3, "singular": 4}   # VISTAF_MOTIONST_*, values of the `status` field
NPRESSURE, NPRESSUREFRAME = 16, 12                                  # VISTAF_NPRESSURE, VISTAF_NPRESSUREFRAME (include/vistaf_pressure.h)
# fields of a pressure row in the order of the VISTAF_PRESSURE_* indices (13..15 are reserved), and of a frame row (VISTAF_PRESSUREFRAME_*)
PRESSURE_NAMES = ["pixels", "force_model_N", "tensile_model_N", "force_N", "mean_kPa", "peak_kPa", "peak_index", "cop_x", "cop_y", "offset_x_mm",
                  "offset_y_mm", "peak_over_mean", "edge_share"]
PRESSURE_FRAME_NAMES = ["contacts", "force_model_N", "tensile_model_N", "outside_model_N", "scale", "E_effective_MPa", "peak_kPa", "peak_index",
                        "peak_row", "cop_x", "cop_y", "status"]
ALIGN_NINFO = 12        # doubles per frame record of vistaf_align_batch (VISTAF_ALIGN_NINFO, include/vistaf_align.h)

FMT_GRAY_U8, FMT_BGR_U8, FMT_GRAY_F16, FMT_BGR_F16 = 0, 1, 2, 3
FRAME_OK, FRAME_EMPTY_RELIABLE, FRAME_QUEUE_OVERFLOW, FRAME_NO_CARRIER = 0, 1, 2, 3
CURVE_TYPES = {"linear0": 0, "linear": 1, "poly2": 2, "sat_exp": 3, "growth": 4, "hinge_saturating": 5}

EXPORTS = [
    "vistaf_ftp_abi_version", "vistaf_ftp_last_error", "vistaf_ftp_default_config", "vistaf_ftp_create",
    "vistaf_ftp_set_reference", "vistaf_ftp_get_reference_info", "vistaf_ftp_predict_batch", "vistaf_ftp_predict_pairs",
    "vistaf_ftp_get_pair_info", "vistaf_ftp_contacts",
    "vistaf_ftp_get_intermediate", "vistaf_ftp_stage_count", "vistaf_ftp_stage_name",
    "vistaf_ftp_enable_stage_timing", "vistaf_ftp_get_stage_times", "vistaf_ftp_destroy",
    "vistaf_depth_map_to_volume", "vistaf_predict_force_from_volume",
]
# csrc/test_hooks.h: kernel tier selection / debug planes for the parity tests, and the selection, fit and blur launchers on planes of the test's own
TEST_EXPORTS = ["vistaf_ftp_test_set", "vistaf_ftp_test_select", "vistaf_ftp_test_select_instance", "vistaf_ftp_test_select_chained", "vistaf_ftp_test_polyfit", "vistaf_ftp_test_gauss",
                "vistaf_ftp_test_chamfer", "vistaf_ftp_test_scratch_regions", "vistaf_ftp_test_cc_label", "vistaf_ftp_test_cc_largest",
                "vistaf_ftp_test_chamfer_dispatch", "vistaf_ftp_test_blob_filter", "vistaf_ftp_test_dft_full_mag"]
TEMP_EXPORTS = ["vistaf_tempseg_default_config", "vistaf_tempseg_create", "vistaf_tempseg_destroy", "vistaf_tempseg_segment",
                "vistaf_temp_feature_planes", "vistaf_temp_color_support",
                "vistaf_temp_clamp_map", "vistaf_temp_inpaint_map", "vistaf_temp_fuse_maps", "vistaf_temp_oriented_blur"]   # include/vistaf_temp.h
TEMPSEG_NINFO = 16
TEMPMODEL_EXPORTS = ["vistaf_tmodel_create", "vistaf_tmodel_destroy", "vistaf_tmodel_predict_maps", "vistaf_tmodel_predict_rows"]   # include/vistaf_tempmodel.h
TSENSOR_EXPORTS = ["vistaf_tsensor_default_config", "vistaf_tsensor_create", "vistaf_tsensor_destroy", "vistaf_tsensor_predict",
                   "vistaf_tsensor_stats_create", "vistaf_tsensor_stats_destroy", "vistaf_tsensor_map_statistics"]   # include/vistaf_tempsensor.h
TSENSOR_NINFO, TSENSOR_NMASKS, TSENSOR_NSTATS = TEMPSEG_NINFO + 4, 5, 6
TRACK_EXPORTS = ["vistaf_track_create", "vistaf_track_update", "vistaf_track_reset", "vistaf_track_destroy"]   # include/vistaf_track.h
SHAPE_EXPORTS = ["vistaf_shape_create", "vistaf_shape_measure", "vistaf_shape_destroy"]   # include/vistaf_shape.h
TAXEL_EXPORTS = ["vistaf_taxel_create", "vistaf_taxel_measure", "vistaf_taxel_layout_info", "vistaf_taxel_destroy"]   # include/vistaf_taxel.h
THERMAL_EXPORTS = ["vistaf_thermal_create", "vistaf_thermal_register", "vistaf_thermal_measure", "vistaf_thermal_destroy"]   # include/vistaf_thermal.h
TEMPORAL_EXPORTS = ["vistaf_temporal_create", "vistaf_temporal_update", "vistaf_temporal_state", "vistaf_temporal_reset",
                    "vistaf_temporal_destroy"]   # include/vistaf_temporal.h
CLOUD_EXPORTS = ["vistaf_cloud_create", "vistaf_cloud_measure", "vistaf_cloud_destroy"]   # include/vistaf_cloud.h
MOTION_EXPORTS = ["vistaf_motion_create", "vistaf_motion_update", "vistaf_motion_reset", "vistaf_motion_destroy"]   # include/vistaf_motion.h
PRESSURE_EXPORTS = ["vistaf_pressure_create", "vistaf_pressure_measure", "vistaf_pressure_destroy"]   # include/vistaf_pressure.h
ALIGN_EXPORTS = [            # include/vistaf_align.h
    "vistaf_align_default_config", "vistaf_align_create", "vistaf_align_destroy", "vistaf_align_geometry",
    "vistaf_align_set_reference", "vistaf_align_batch",
]


class Curve(ctypes.Structure):
    _fields_ = [("type", ctypes.c_int32), ("reserved", ctypes.c_int32),
                ("a", ctypes.c_double), ("b", ctypes.c_double), ("c", ctypes.c_double)]


_INT_FIELDS = [
    "patch_half_width_bins", "dc_exclusion", "fft_pad_px", "roi_erode_px", "apod_taper_px", "reliable_edge_margin_px",
    "poly_order", "frontier_zero_band_px", "valid_close_kernel", "valid_close_iters", "bad_pixel_enable",
    "bad_dilate_ksize", "bad_dilate_iters", "bad_inpaint_radius", "dilate_kernel_size", "dilate_iters", "n_fft_peaks",
    "plane_order_for_removal", "irls_iters", "hole_neighborhood_px", "hole_min_dist_px", "inpaint_radius",
]
_DBL_FIELDS = [
    "pre_blur_sigma_px", "amp_valid_percentile", "quality_smooth_sigma_px", "reliable_smooth_sigma_px", "illum_sigma_px",
    "bad_intensity_percentile", "bad_gradient_percentile", "contact_core_percentile", "contact_percentile",
    "min_contact_frac", "max_contact_frac", "unreliable_smooth_sigma_px", "contact_blob_min_peak_mm",
    "contact_blob_min_peak_rel_frac", "peak_max_dy_from_center", "irls_c", "grating_pitch_mm", "depth_eps_mm", "hole_known_fraction",
]


class CConfig(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int32) for n in _INT_FIELDS] + [(n, ctypes.c_double) for n in _DBL_FIELDS]


class CTempFuseConfig(ctypes.Structure):
    _fields_ = [(n, ctypes.c_double) for n in ("color_t_min", "color_t_max", "color_guard_band", "switch_margin_c", "final_t_min", "final_t_max")]


class CTempSegConfig(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int32) for n in ("seg_band_radius", "seg_dc_exclusion", "seg_illum_sigma", "sat_thresh_gray", "sat_dilate_ksize",
                                                "post_close_kx", "post_close_ky", "post_open_kx", "post_open_ky", "n_peaks")] + \
               [("seg_peak_max_dy_from_center", ctypes.c_double)]


class CTSensorConfig(ctypes.Structure):
    _fields_ = [("seg", CTempSegConfig), ("fuse", CTempFuseConfig)] + \
               [(n, ctypes.c_int32) for n in ("blur_ksize", "color_support_dilate", "wide_inpaint_radius", "color_inpaint_radius")] + \
               [(n, ctypes.c_double) for n in ("color_chroma_min", "color_clamp_pad", "smooth_sigma_across", "smooth_sigma_along")]


_lib = None


def load():
    """Load libvistaf_ftp.so; raises RuntimeError (never falls back) when it is missing."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f"{LIB_PATH} is missing: build it with `python __graft_entry__.py` (hipcc --offload-arch=gfx950). "
            "This package has no CPU path."
        )
    lib = ctypes.CDLL(LIB_PATH)
    vp, ci, cd = ctypes.c_void_p, ctypes.c_int, ctypes.c_double
    lib.vistaf_ftp_abi_version.restype = ci
    lib.vistaf_ftp_last_error.restype = ctypes.c_char_p
    lib.vistaf_ftp_default_config.argtypes = [ctypes.POINTER(CConfig)]
    lib.vistaf_ftp_create.argtypes = [ctypes.POINTER(CConfig), ci, ci, ci, ci, ci, ci, ctypes.POINTER(Curve), ci,
                                      ctypes.POINTER(Curve), ctypes.POINTER(vp)]
    lib.vistaf_ftp_set_reference.argtypes = [vp, vp, ci, vp]
    lib.vistaf_ftp_get_reference_info.argtypes = [vp, ctypes.POINTER(cd)]
    lib.vistaf_ftp_predict_batch.argtypes = [vp, vp, ci, ci, vp, vp, vp, vp, vp]
    lib.vistaf_ftp_predict_pairs.argtypes = [vp, vp, vp, ci, ci, vp, vp, vp, vp, vp]
    lib.vistaf_ftp_get_pair_info.argtypes = [vp, ci, ctypes.POINTER(cd), vp]
    lib.vistaf_ftp_contacts.argtypes = [vp, ci, ci, vp, vp, vp, vp]
    lib.vistaf_ftp_get_intermediate.argtypes = [vp, ctypes.c_char_p, vp, ci, ctypes.POINTER(ctypes.c_size_t), vp]
    lib.vistaf_ftp_stage_count.restype = ci
    lib.vistaf_ftp_stage_name.restype = ctypes.c_char_p
    lib.vistaf_ftp_stage_name.argtypes = [ci]
    lib.vistaf_ftp_enable_stage_timing.argtypes = [vp, ci]
    lib.vistaf_ftp_get_stage_times.argtypes = [vp, ctypes.POINTER(ctypes.c_float), ci]
    lib.vistaf_ftp_destroy.argtypes = [vp]
    lib.vistaf_ftp_destroy.restype = None
    lib.vistaf_depth_map_to_volume.argtypes = [vp, vp, ci, ci, ci, cd, cd, vp, vp]
    lib.vistaf_predict_force_from_volume.argtypes = [ctypes.POINTER(Curve), cd, ctypes.POINTER(cd)]
    lib.vistaf_ftp_test_set.argtypes = [vp, ctypes.c_char_p, ci]
    lib.vistaf_ftp_test_select.argtypes = [vp, vp, ctypes.c_size_t, vp, ci, vp, ci, vp, vp, ci, ci, ci, vp]
    lib.vistaf_ftp_test_select_instance.argtypes = [ci, ci, ci, ci]
    lib.vistaf_ftp_test_select_chained.argtypes = [vp, vp, ctypes.c_size_t, ci, vp, ci, vp, vp, ci, ci, vp]
    lib.vistaf_ftp_test_polyfit.argtypes = [vp, vp, ci, ci, ctypes.c_float, ci, ci, vp, vp, ci, ci, ci, ci, vp]
    lib.vistaf_ftp_test_gauss.argtypes = [vp, vp, cd, ci, ci, ci, vp]
    lib.vistaf_ftp_test_chamfer.argtypes = [vp, ci, ci, vp, vp, ci, ci, ci, ci, vp]
    lib.vistaf_ftp_test_cc_label.argtypes = [vp, vp, ci, ci, ci, ci, vp]
    lib.vistaf_ftp_test_cc_largest.argtypes = [vp, vp, vp, ci, ci, ci, vp]
    lib.vistaf_ftp_test_chamfer_dispatch.argtypes = [vp, ci, ci, vp, vp, ci, ci, ci, ci, vp]
    lib.vistaf_ftp_test_blob_filter.argtypes = [vp, vp, vp, vp, cd, cd, vp, ci, ci, vp]
    lib.vistaf_ftp_test_dft_full_mag.argtypes = [vp, vp, vp, vp, vp, ci, ci, ci, ci, ci, vp]
    szp = ctypes.POINTER(ctypes.c_size_t)
    lib.vistaf_ftp_test_scratch_regions.argtypes = [ctypes.c_char_p, ci, ci, ci, ci, ci, ctypes.c_char_p, szp, szp, szp, szp]
    lib.vistaf_tempseg_default_config.argtypes = [ctypes.POINTER(CTempSegConfig)]
    lib.vistaf_tempseg_create.argtypes = [ctypes.POINTER(CTempSegConfig), ci, ci, ctypes.POINTER(vp)]
    lib.vistaf_tempseg_destroy.argtypes = [vp]
    lib.vistaf_tempseg_destroy.restype = None
    lib.vistaf_tempseg_segment.argtypes = [vp, vp, vp, vp, vp, vp, vp, ctypes.POINTER(cd), vp]
    lib.vistaf_temp_feature_planes.argtypes = [vp, vp, ci, vp, vp, vp, vp, vp]
    lib.vistaf_temp_color_support.argtypes = [vp, vp, vp, vp, vp, vp, cd, ci, vp, vp, vp]
    lib.vistaf_temp_clamp_map.argtypes = [vp, vp, vp, cd, cd, vp, vp]
    lib.vistaf_temp_inpaint_map.argtypes = [vp, vp, vp, ci, vp, vp]
    lib.vistaf_temp_fuse_maps.argtypes = [vp, vp, vp, vp, ctypes.POINTER(CTempFuseConfig), vp, vp, ctypes.POINTER(ctypes.c_int64), vp]
    lib.vistaf_temp_oriented_blur.argtypes = [vp, vp, vp, cd, cd, cd, vp, vp]
    i32p, dp = ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(cd)
    lib.vistaf_tmodel_create.argtypes = [ci, i32p, dp, dp, ci, ci, ci, i32p, dp, cd, ci, dp, dp, cd, cd, ci, ctypes.POINTER(vp)]
    lib.vistaf_tmodel_destroy.argtypes = [vp]
    lib.vistaf_tmodel_destroy.restype = None
    lib.vistaf_tmodel_predict_maps.argtypes = [ci, ctypes.POINTER(vp), ctypes.POINTER(vp), ctypes.POINTER(vp), ctypes.POINTER(vp), ctypes.c_int64,
                                               ctypes.c_int64, vp]
    lib.vistaf_tmodel_predict_rows.argtypes = [vp, vp, ci, ctypes.c_int64, vp, vp]
    lib.vistaf_tsensor_default_config.argtypes = [ctypes.POINTER(CTSensorConfig)]
    lib.vistaf_tsensor_create.argtypes = [ctypes.POINTER(CTSensorConfig), ci, ci, vp, vp, ctypes.POINTER(vp)]
    lib.vistaf_tsensor_destroy.argtypes = [vp]
    lib.vistaf_tsensor_destroy.restype = None
    lib.vistaf_tsensor_predict.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, ctypes.POINTER(cd), vp, ctypes.POINTER(cd), vp]
    lib.vistaf_tsensor_stats_create.argtypes = [ci, ci, ctypes.POINTER(vp)]
    lib.vistaf_tsensor_stats_destroy.argtypes = [vp]
    lib.vistaf_tsensor_stats_destroy.restype = None
    lib.vistaf_tsensor_map_statistics.argtypes = [vp, vp, vp, vp, ctypes.POINTER(cd), vp]
    lib.vistaf_track_create.argtypes = [ci, ci, ci, ci, cd, ctypes.POINTER(vp)]
    lib.vistaf_track_update.argtypes = [vp, vp, vp, vp, ci, vp, vp, vp]
    lib.vistaf_track_reset.argtypes = [vp]
    lib.vistaf_track_destroy.argtypes = [vp]
    lib.vistaf_track_destroy.restype = None
    lib.vistaf_shape_create.argtypes = [ci, ci, ci, ci, cd, ctypes.POINTER(vp)]
    lib.vistaf_shape_measure.argtypes = [vp, vp, vp, vp, vp, vp, ctypes.c_float, ci, vp, vp]
    lib.vistaf_shape_destroy.argtypes = [vp]
    lib.vistaf_shape_destroy.restype = None
    lib.vistaf_taxel_create.argtypes = [ci, ci, ci, vp, ci, cd, cd, ctypes.POINTER(vp)]
    lib.vistaf_taxel_measure.argtypes = [vp, vp, vp, vp, vp, ctypes.c_float, ci, vp, vp, vp]
    lib.vistaf_taxel_layout_info.argtypes = [vp, vp]
    lib.vistaf_taxel_destroy.argtypes = [vp]
    lib.vistaf_taxel_destroy.restype = None
    lib.vistaf_thermal_create.argtypes = [ci, ci, ci, ci, ci, ci, ci, ci, ci, ci, ctypes.POINTER(vp)]
    lib.vistaf_thermal_register.argtypes = [vp, vp, vp, ci, vp, vp]
    lib.vistaf_thermal_measure.argtypes = [vp, vp, vp, vp, vp, vp, vp, ctypes.c_float, ci, vp, vp, vp]
    lib.vistaf_thermal_destroy.argtypes = [vp]
    lib.vistaf_thermal_destroy.restype = None
    lib.vistaf_temporal_create.argtypes = [ci, ci, ci, cd, cd, cd, cd, ctypes.POINTER(vp)]
    lib.vistaf_temporal_update.argtypes = [vp, vp, vp, vp, ci, vp, vp, vp, vp]
    lib.vistaf_temporal_state.argtypes = [vp, vp, vp, vp, vp, vp, vp]
    lib.vistaf_temporal_reset.argtypes = [vp]
    lib.vistaf_temporal_destroy.argtypes = [vp]
    lib.vistaf_temporal_destroy.restype = None
    lib.vistaf_cloud_create.argtypes = [ci, ci, ci, ctypes.c_int64, ci, cd, cd, ctypes.POINTER(vp)]
    lib.vistaf_cloud_measure.argtypes = [vp, vp, vp, vp, vp, ctypes.c_float, ci, vp, vp, vp, vp, vp, vp]
    lib.vistaf_cloud_destroy.argtypes = [vp]
    lib.vistaf_cloud_destroy.restype = None
    lib.vistaf_motion_create.argtypes = [ci, ci, ci, ci, ci, cd, ci, ci, ctypes.POINTER(vp)]
    lib.vistaf_motion_update.argtypes = [vp, vp, vp, vp, vp, vp, vp, ctypes.c_float, ci, vp, vp, vp]
    lib.vistaf_motion_reset.argtypes = [vp]
    lib.vistaf_motion_destroy.argtypes = [vp]
    lib.vistaf_motion_destroy.restype = None
    lib.vistaf_pressure_create.argtypes = [ci, ci, ci, ci, ci, cd, cd, cd, ctypes.POINTER(vp)]
    lib.vistaf_pressure_measure.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, ctypes.c_float, ci, vp, vp, vp, vp]
    lib.vistaf_pressure_destroy.argtypes = [vp]
    lib.vistaf_pressure_destroy.restype = None
    for fn in (EXPORTS + ALIGN_EXPORTS + TEST_EXPORTS + TEMP_EXPORTS + TEMPMODEL_EXPORTS + TSENSOR_EXPORTS + TRACK_EXPORTS + SHAPE_EXPORTS + TAXEL_EXPORTS +
               THERMAL_EXPORTS + TEMPORAL_EXPORTS + CLOUD_EXPORTS + MOTION_EXPORTS + PRESSURE_EXPORTS):
        getattr(lib, fn)
    _lib = lib
    return lib


def check(rc: int):
    if rc != 0:
        msg = load().vistaf_ftp_last_error().decode("utf-8", "replace")
        if rc == -1:
            raise ValueError(msg)
        raise RuntimeError(f"vistaf_ftp error {rc}: {msg}")
