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
NOUTLINE = 24           # doubles per row of the contact outline read-out (VISTAF_NOUTLINE, include_ext/vistaf_outline.h)
# fields of an outline row in the order of the VISTAF_OUTLINE_* indices; 20..23 are reserved
OUTLINE_NAMES = ["pixels", "pieces", "holes", "edges", "edges_all", "perimeter_mm", "enclosed_pixels", "corners", "corners_written", "hull_vertices",
                 "hull_area_mm2", "solidity", "max_feret_mm", "max_feret_angle_rad", "min_feret_mm", "box_cx", "box_cy", "box_length_mm",
                 "box_width_mm", "box_angle_rad"]
NTEXTURE = 40           # doubles per row of the surface texture read-out (VISTAF_NTEXTURE, include_ext/vistaf_texture.h)
# fields of a texture row in the order of the VISTAF_TEXTURE_* indices; 34..39 are reserved
TEXTURE_NAMES = ["eval_pixels", "form_status", "form_c0", "form_c1", "form_c2", "form_c3", "form_c4", "form_c5", "sa_mm", "sq_mm", "ssk", "sku",
                 "sp_mm", "sv_mm", "sz_mm", "sp_pixel", "sv_pixel", "grad_pixels", "sdq", "sdr", "grad_dir_x", "grad_dir_y", "coherence",
                 "acf_valid_lags", "lobe_lags", "lobe_status", "sal_mm", "sal_lag_x", "sal_lag_y", "rmax_mm", "str", "pitch_mm", "pitch_acf",
                 "profile_samples"]
TEXTURE_FORM = {"ok": 0, "none": 1, "flat": 2}                       # VISTAF_TEXTUREFORM_*, values of the `form_status` field
TEXTURE_MIN_LAG, TEXTURE_MAX_LAG = 2, 31                             # VISTAF_TEXTURE_MIN_LAG, _MAX_LAG
NMATCH = 24             # doubles per row of the indenter match read-out (VISTAF_NMATCH, include_ext/vistaf_match.h)
# fields of a match row in the order of the VISTAF_MATCH_* indices; 23 is reserved
MATCH_NAMES = ["status", "flags", "label", "template", "class", "rotation", "shift_x", "shift_y", "score", "angle_rad", "x_px", "y_px", "offset_x_mm",
               "offset_y_mm", "second_class", "second_score", "margin", "rot_contrast", "scale", "base_mm", "resid_rms_mm", "support_pixels",
               "valid_shifts"]
MATCH_STATUS = {"ok": 0, "no_pixels": 1, "no_scale": 2, "no_support": 3}              # VISTAF_MATCHST_*, values of the `status` field
MATCH_FLAGS = {"clipped": 1, "border_shift": 2, "weak": 4, "ambiguous": 8}            # VISTAF_MATCHFL_*, bits of the `flags` field
# VISTAF_MATCH_MAGIC, _HEADER_INTS, _MIN_P, _MAX_P, _MAX_R, _MAX_T, _MAX_SYMMETRY, _MAX_SHIFT, _MAX_ROWS
MATCH_MAGIC, MATCH_HEADER_INTS, MATCH_MIN_P, MATCH_MAX_P, MATCH_MAX_R, MATCH_MAX_T, MATCH_MAX_SYMMETRY, MATCH_MAX_SHIFT, MATCH_MAX_ROWS = \
    0x31424d56, 16, 5, 33, 64, 64, 8, 8, 2048
NCENTRELINE = 40        # doubles per row of the centreline read-out (VISTAF_NCENTRELINE, include_ext/vistaf_centreline.h)
# fields of a centreline row in the order of the VISTAF_CENTRELINE_* indices; 37..39 are reserved
CENTRELINE_NAMES = ["pixels", "skeleton_pixels", "thinning_passes", "end_pixels", "branch_pixels", "stations", "stations_written", "status", "a_x",
                    "a_y", "b_x", "b_y", "path_length_mm", "length_mm", "chord_mm", "tortuosity", "sagitta_mm", "sagitta_station",
                    "interior_stations", "width_mean_mm", "width_min_mm", "width_min_station", "width_max_mm", "width_max_station", "width_seed_mm",
                    "elongation", "a_tx", "a_ty", "b_tx", "b_ty", "a_at_border", "b_at_border", "depth_mean_mm", "depth_a_mm", "depth_b_mm",
                    "depth_peak_mm", "depth_peak_station"]
# VISTAF_CLST_*: values (ok, no_pixels, point) and flags (branched, truncated) of the `status` field
CENTRELINE_STATUS = {"ok": 0, "no_pixels": 1, "point": 2, "branched": 8, "truncated": 16}
NLOBE, NLOBEROW, LOBES_MAX = 16, 12, 64                              # VISTAF_NLOBE, VISTAF_NLOBEROW, VISTAF_LOBES_MAX (include_ext/vistaf_lobes.h)
# fields of a lobe record in the order of the VISTAF_LOBE_* indices, and of a row record (VISTAF_LOBEROW_*; 9..11 are reserved)
LOBE_NAMES = ["x", "y", "depth_mm", "prominence_mm", "saddle_x", "saddle_y", "saddle_depth_mm", "neighbour", "pixels", "contact_pixels", "area_mm2",
              "volume_cm3", "centroid_x", "centroid_y", "force_share_N", "basins"]
LOBE_ROW_NAMES = ["pixels", "raw_maxima", "peaks", "peaks_written", "status", "threshold_mm", "separation_mm", "deepest_saddle_mm", "next_prominence_mm"]
LOBE_STATUS = {"ok": 0, "no_pixels": 1, "truncated": 16}              # VISTAF_LOBEST_*: values (ok, no_pixels) and flag (truncated) of `status`
ALIGN_NINFO = 12        # doubles per frame record of vistaf_align_batch (VISTAF_ALIGN_NINFO, include/vistaf_align.h)

FMT_GRAY_U8, FMT_BGR_U8, FMT_GRAY_F16, FMT_BGR_F16 = 0, 1, 2, 3
# the camera-native layouts (VISTAF_FMT_*, include/vistaf_ftp.h)
FMT_RGB_U8, FMT_BGRA_U8, FMT_RGBA_U8, FMT_YUYV_U8, FMT_UYVY_U8, FMT_NV12_U8 = 4, 5, 6, 7, 8, 9
FMT_BAYER_RGGB_U8, FMT_BAYER_GRBG_U8, FMT_BAYER_GBRG_U8, FMT_BAYER_BGGR_U8 = 10, 11, 12, 13
# the name a caller gives as `format=` -> code; the header's VISTAF_FMT_<NAME>_U8 is the name in capitals (the two F16 formats keep their suffix)
FORMATS = {"gray": 0, "bgr": 1, "gray_f16": 2, "bgr_f16": 3, "rgb": 4, "bgra": 5, "rgba": 6, "yuyv": 7, "uyvy": 8, "nv12": 9,
           "bayer_rggb": 10, "bayer_grbg": 11, "bayer_gbrg": 12, "bayer_bggr": 13}
FRAME_OK, FRAME_EMPTY_RELIABLE, FRAME_QUEUE_OVERFLOW, FRAME_NO_CARRIER = 0, 1, 2, 3
CURVE_TYPES = {"linear0": 0, "linear": 1, "poly2": 2, "sat_exp": 3, "growth": 4, "hinge_saturating": 5}

TEMPSEG_NINFO = 16
TSENSOR_NINFO, TSENSOR_NMASKS, TSENSOR_NSTATS = TEMPSEG_NINFO + 4, 5, 6


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


class AlignConfig(ctypes.Structure):
    _fields_ = [("apply_global_shift", ctypes.c_int32), ("use_ecc", ctypes.c_int32), ("ecc_iters", ctypes.c_int32), ("gray_coeffs", ctypes.c_int32),
                ("ecc_eps", ctypes.c_double), ("ecc_gauss_sigma", ctypes.c_double), ("shift_blur_sigma", ctypes.c_double)]


vp, ci, cd, cf, cs, sz, i32, i64, P = (ctypes.c_void_p, ctypes.c_int, ctypes.c_double, ctypes.c_float, ctypes.c_char_p, ctypes.c_size_t, ctypes.c_int32,
                                       ctypes.c_int64, ctypes.POINTER)
# The C ABI, stated once: every exported function -> (restype, argtypes), grouped by the header that declares it and in its order.  load()
# applies the table; tests/test_abi_surface.py holds it against the prototypes.  A device pointer or a stream is vp, a handle vp, its slot P(vp).
SIGNATURES = {
    "EXPORTS": {        # include/vistaf_ftp.h
        "vistaf_ftp_abi_version": (ci, []),
        "vistaf_ftp_last_error": (cs, []),
        "vistaf_ftp_default_config": (ci, [P(CConfig)]),
        "vistaf_ftp_create": (ci, [P(CConfig), ci, ci, ci, ci, ci, ci, P(Curve), ci, P(Curve), P(vp)]),
        "vistaf_ftp_set_reference": (ci, [vp, vp, ci, vp]),
        "vistaf_ftp_get_reference_info": (ci, [vp, P(cd)]),
        "vistaf_ftp_predict_batch": (ci, [vp, vp, ci, ci, vp, vp, vp, vp, vp]),
        "vistaf_ftp_predict_pairs": (ci, [vp, vp, vp, ci, ci, vp, vp, vp, vp, vp]),
        "vistaf_ftp_get_pair_info": (ci, [vp, ci, P(cd), vp]),
        "vistaf_ftp_contacts": (ci, [vp, ci, ci, vp, vp, vp, vp]),
        "vistaf_ftp_get_intermediate": (ci, [vp, cs, vp, ci, P(sz), vp]),
        "vistaf_ftp_stage_count": (ci, []),
        "vistaf_ftp_stage_name": (cs, [ci]),
        "vistaf_ftp_enable_stage_timing": (ci, [vp, ci]),
        "vistaf_ftp_get_stage_times": (ci, [vp, P(cf), ci]),
        "vistaf_ftp_destroy": (None, [vp]),
        "vistaf_depth_map_to_volume": (ci, [vp, vp, ci, ci, ci, cd, cd, vp, vp]),
        "vistaf_predict_force_from_volume": (ci, [P(Curve), cd, P(cd)]),
    },
    "ALIGN_EXPORTS": {        # include/vistaf_align.h
        "vistaf_align_default_config": (None, [P(AlignConfig)]),
        "vistaf_align_create": (ci, [P(AlignConfig), ci, ci, ci, ci, ci, ci, P(vp)]),
        "vistaf_align_destroy": (None, [vp]),
        "vistaf_align_geometry": (ci, [vp] + [P(i32)] * 9),
        "vistaf_align_set_reference": (ci, [vp, vp, vp, vp]),
        "vistaf_align_batch": (ci, [vp, vp, ci, vp, vp, vp]),
    },
    "TEST_EXPORTS": {        # csrc/test_hooks.h
        "vistaf_ftp_test_set": (ci, [vp, cs, ci]),
        "vistaf_ftp_test_select": (ci, [vp, vp, sz, vp, ci, vp, ci, vp, vp, ci, ci, ci, vp]),
        "vistaf_ftp_test_select_instance": (ci, [ci, ci, ci, ci]),
        "vistaf_ftp_test_select_chained": (ci, [vp, vp, sz, ci, vp, ci, vp, vp, ci, ci, vp]),
        "vistaf_ftp_test_polyfit": (ci, [vp, vp, ci, ci, cf, ci, ci, vp, vp, ci, ci, ci, ci, vp]),
        "vistaf_ftp_test_gauss": (ci, [vp, vp, cd, ci, ci, ci, vp]),
        "vistaf_ftp_test_chamfer": (ci, [vp, ci, ci, vp, vp, ci, ci, ci, ci, vp]),
        "vistaf_ftp_test_scratch_regions": (ci, [cs, ci, ci, ci, ci, ci, cs, P(sz), P(sz), P(sz), P(sz)]),
        "vistaf_ftp_test_cc_label": (ci, [vp, vp, ci, ci, ci, ci, vp]),
        "vistaf_ftp_test_cc_largest": (ci, [vp, vp, vp, ci, ci, ci, vp]),
        "vistaf_ftp_test_chamfer_dispatch": (ci, [vp, ci, ci, vp, vp, ci, ci, ci, ci, vp]),
        "vistaf_ftp_test_blob_filter": (ci, [vp, vp, vp, vp, cd, cd, vp, ci, ci, vp]),
        "vistaf_ftp_test_unwrap": (ci, [vp, vp, vp, vp, vp, vp, vp, ci, ci, ci, ci, vp]),
        "vistaf_ftp_test_inpaint": (ci, [vp, vp, ci, ci, vp, vp, ci, ci, ci, ci, vp]),
        "vistaf_ftp_test_dft_full_mag": (ci, [vp, vp, vp, vp, vp, ci, ci, ci, ci, ci, vp]),
        "vistaf_ftp_test_top_peaks": (ci, [vp, ci, ci, ci, ci, ci, vp, vp]),
        "vistaf_ftp_test_carrier_choose": (ci, [vp, ci, vp, ci, ci, ci, cd, vp, vp, ci, vp]),
        "vistaf_ftp_test_build_tables": (ci, [vp, vp, ci, ci, ci, ci, ci, ci, ci, ci, ci, vp, vp, vp, vp, vp, vp]),
        "vistaf_ftp_test_build_full_tables": (ci, [vp, vp, ci, ci, ci, ci, ci, vp]),
        "vistaf_ftp_test_dft_forward": (ci, [vp, vp, vp, vp, sz, sz, vp, ci, vp, vp, ci, ci, ci, ci, ci, ci, vp]),
        "vistaf_ftp_test_dft_inverse": (ci, [vp, ci, vp, vp, sz, sz, vp, vp, vp, vp, vp, sz, vp, vp, vp, ci, ci, ci, ci, ci, vp]),
        "vistaf_ftp_test_morph": (ci, [vp, vp, ci, ci, ci, ci, ci, ci, ci, vp, vp, ci, vp]),
        "vistaf_ftp_test_tempseg_plane": (ci, [vp, cs, vp, sz, vp]),
        "vistaf_ftp_test_tempseg_sign": (ci, [vp, cd, vp, vp, vp, P(cd), sz, vp]),
    },
    "TEMP_EXPORTS": {        # include/vistaf_temp.h
        "vistaf_tempseg_default_config": (ci, [P(CTempSegConfig)]),
        "vistaf_tempseg_create": (ci, [P(CTempSegConfig), ci, ci, P(vp)]),
        "vistaf_tempseg_destroy": (None, [vp]),
        "vistaf_tempseg_segment": (ci, [vp, vp, vp, vp, vp, vp, vp, P(cd), vp]),
        "vistaf_temp_feature_planes": (ci, [vp, vp, ci, vp, vp, vp, vp, vp]),
        "vistaf_temp_color_support": (ci, [vp, vp, vp, vp, vp, vp, cd, ci, vp, vp, vp]),
        "vistaf_temp_clamp_map": (ci, [vp, vp, vp, cd, cd, vp, vp]),
        "vistaf_temp_inpaint_map": (ci, [vp, vp, vp, ci, vp, vp]),
        "vistaf_temp_fuse_maps": (ci, [vp, vp, vp, vp, P(CTempFuseConfig), vp, vp, P(i64), vp]),
        "vistaf_temp_oriented_blur": (ci, [vp, vp, vp, cd, cd, cd, vp, vp]),
    },
    "TEMPMODEL_EXPORTS": {        # include/vistaf_tempmodel.h
        "vistaf_tmodel_create": (ci, [ci, P(i32), P(cd), P(cd), ci, ci, ci, P(i32), P(cd), cd, ci, P(cd), P(cd), cd, cd, ci, P(vp)]),
        "vistaf_tmodel_destroy": (None, [vp]),
        "vistaf_tmodel_predict_maps": (ci, [ci, P(vp), P(vp), P(vp), P(vp), i64, i64, vp]),
        "vistaf_tmodel_predict_rows": (ci, [vp, vp, ci, i64, vp, vp]),
    },
    "TSENSOR_EXPORTS": {        # include/vistaf_tempsensor.h
        "vistaf_tsensor_default_config": (ci, [P(CTSensorConfig)]),
        "vistaf_tsensor_create": (ci, [P(CTSensorConfig), ci, ci, vp, vp, P(vp)]),
        "vistaf_tsensor_destroy": (None, [vp]),
        "vistaf_tsensor_predict": (ci, [vp, vp, vp, vp, vp, vp, vp, vp, P(cd), vp, P(cd), vp]),
        "vistaf_tsensor_stats_create": (ci, [ci, ci, P(vp)]),
        "vistaf_tsensor_stats_destroy": (None, [vp]),
        "vistaf_tsensor_map_statistics": (ci, [vp, vp, vp, vp, P(cd), vp]),
    },
    "TRACK_EXPORTS": {        # include/vistaf_track.h
        "vistaf_track_create": (ci, [ci, ci, ci, ci, cd, P(vp)]),
        "vistaf_track_update": (ci, [vp, vp, vp, vp, ci, vp, vp, vp]),
        "vistaf_track_reset": (ci, [vp]),
        "vistaf_track_destroy": (None, [vp]),
    },
    "SHAPE_EXPORTS": {        # include/vistaf_shape.h
        "vistaf_shape_create": (ci, [ci, ci, ci, ci, cd, P(vp)]),
        "vistaf_shape_measure": (ci, [vp, vp, vp, vp, vp, vp, cf, ci, vp, vp]),
        "vistaf_shape_destroy": (None, [vp]),
    },
    "TAXEL_EXPORTS": {        # include/vistaf_taxel.h
        "vistaf_taxel_create": (ci, [ci, ci, ci, vp, ci, cd, cd, P(vp)]),
        "vistaf_taxel_measure": (ci, [vp, vp, vp, vp, vp, cf, ci, vp, vp, vp]),
        "vistaf_taxel_layout_info": (ci, [vp, vp]),
        "vistaf_taxel_destroy": (None, [vp]),
    },
    "THERMAL_EXPORTS": {        # include/vistaf_thermal.h
        "vistaf_thermal_create": (ci, [ci, ci, ci, ci, ci, ci, ci, ci, ci, ci, P(vp)]),
        "vistaf_thermal_register": (ci, [vp, vp, vp, ci, vp, vp]),
        "vistaf_thermal_measure": (ci, [vp, vp, vp, vp, vp, vp, vp, cf, ci, vp, vp, vp]),
        "vistaf_thermal_destroy": (None, [vp]),
    },
    "TEMPORAL_EXPORTS": {        # include/vistaf_temporal.h
        "vistaf_temporal_create": (ci, [ci, ci, ci, cd, cd, cd, cd, P(vp)]),
        "vistaf_temporal_update": (ci, [vp, vp, vp, vp, ci, vp, vp, vp, vp]),
        "vistaf_temporal_state": (ci, [vp, vp, vp, vp, vp, vp, vp]),
        "vistaf_temporal_reset": (ci, [vp]),
        "vistaf_temporal_destroy": (None, [vp]),
    },
    "CLOUD_EXPORTS": {        # include/vistaf_cloud.h
        "vistaf_cloud_create": (ci, [ci, ci, ci, i64, ci, cd, cd, P(vp)]),
        "vistaf_cloud_measure": (ci, [vp, vp, vp, vp, vp, cf, ci, vp, vp, vp, vp, vp, vp]),
        "vistaf_cloud_destroy": (None, [vp]),
    },
    "MOTION_EXPORTS": {        # include/vistaf_motion.h
        "vistaf_motion_create": (ci, [ci, ci, ci, ci, ci, cd, ci, ci, P(vp)]),
        "vistaf_motion_update": (ci, [vp, vp, vp, vp, vp, vp, vp, cf, ci, vp, vp, vp]),
        "vistaf_motion_reset": (ci, [vp]),
        "vistaf_motion_destroy": (None, [vp]),
    },
    "PRESSURE_EXPORTS": {        # include/vistaf_pressure.h
        "vistaf_pressure_create": (ci, [ci, ci, ci, ci, ci, cd, cd, cd, P(vp)]),
        "vistaf_pressure_measure": (ci, [vp, vp, vp, vp, vp, vp, vp, vp, cf, ci, vp, vp, vp, vp]),
        "vistaf_pressure_destroy": (None, [vp]),
    },
}
# csrc/test_hooks_masks.h: the test entry points of the binary-mask chains, a table of their own beside the one above (load() applies both;
# tests/test_mask_chains.py holds it against that header)
MASK_CHAIN_SIGNATURES = {
    "vistaf_ftp_test_mask_chain_fits": (ci, [ci, ci, ci, ci, ci, ci]),
    "vistaf_ftp_test_bad_chain": (ci, [vp, vp, vp, vp, vp, ci, ci, vp, vp, ci, ci, ci, ci, vp]),
    "vistaf_ftp_test_reliable_chain": (ci, [vp, vp, vp, ci, ci, ci, vp, vp, vp, vp, ci, ci, ci, ci, vp]),
    "vistaf_ftp_test_contact_chain": (ci, [vp, vp, vp, vp, cd, cd, ci, ci, vp, vp, vp, vp, ci, ci, ci, ci, vp]),
}
# csrc/test_hooks_dft.h: the demodulation launchers with a kernel variant, and what a shape takes (tests/test_dft_staged.py holds the table
# against that header)
DFT_STAGED_SIGNATURES = {
    "vistaf_ftp_test_dft_forward_v": (ci, [vp, vp, vp, vp, sz, sz, vp, ci, vp, vp, ci, ci, ci, ci, ci, ci, ci, vp]),
    "vistaf_ftp_test_dft_inverse_v": (ci, [vp, ci, vp, vp, sz, sz, vp, vp, vp, vp, vp, sz, vp, vp, vp, ci, ci, ci, ci, ci, ci, vp]),
    "vistaf_ftp_test_dft_staged_fits": (ci, [ci, ci, ci, ci, ci]),
}
# csrc/test_hooks_gauss.h: the plain blur with a kernel variant, and what a blur takes (tests/test_gauss_strip.py holds the table against that header)
GAUSS_STRIP_SIGNATURES = {
    "vistaf_ftp_test_gauss_variant": (ci, [vp, vp, cd, ci, ci, ci, ci, vp]),
    "vistaf_ftp_test_gauss_strip_fits": (ci, [ci, ci, ci]),
}
# csrc/test_hooks_fit.h: the IRLS fit through the window kernel, alone and as a chained pair, and the instance a frame size takes
# (tests/test_fit_window.py holds the table against that header)
FIT_WINDOW_SIGNATURES = {
    "vistaf_ftp_test_polyfit_window": (ci, [vp, vp, ci, ci, cf, ci, ci, vp, vp, ci, ci, ci, ci, vp, vp]),
    "vistaf_ftp_test_polyfit_chain": (ci, [vp, vp, ci, ci, ci, cf, ci, ci, ci, vp, vp, vp, ci, ci, ci, ci, vp, vp]),
    "vistaf_ftp_test_polyfit_window_instance": (ci, [ci, ci, ci]),
}
# include_ext/vistaf_outline.h: the contact outline read-out, two plain functions outside the drop-in boundary of include/*.h, in a table of
# their own as well (tests/test_outlines.py holds it against that header)
OUTLINE_SIGNATURES = {
    "vistaf_outline_workspace_bytes": (ci, [ci, ci, ci, ci, P(sz)]),
    "vistaf_outline_measure": (ci, [vp, vp, vp, vp, ci, ci, ci, ci, ci, vp, vp, vp, vp, sz, vp]),
}
# include_ext/vistaf_texture.h: the surface texture read-out, the same pattern (tests/test_textures.py holds it against that header)
TEXTURE_SIGNATURES = {
    "vistaf_texture_workspace_bytes": (ci, [ci, ci, ci, ci, ci, P(sz)]),
    "vistaf_texture_measure": (ci, [vp, vp, vp, vp, vp, cf, cd, ci, ci, cd, cd, ci, ci, ci, ci, vp, vp, vp, vp, sz, vp]),
}
# include_ext/vistaf_match.h: the indenter match read-out, four plain functions, the same pattern (tests/test_matches.py holds it against that header)
MATCH_SIGNATURES = {
    "vistaf_match_bank_bytes": (ci, [ci, ci, ci, P(i32), P(sz)]),
    "vistaf_match_build_bank": (ci, [P(cf), P(i32), P(i32), ci, ci, ci, cd, vp, sz]),
    "vistaf_match_workspace_bytes": (ci, [ci, ci, ci, ci, ci, ci, ci, P(sz)]),
    "vistaf_match_measure": (ci, [vp, vp, vp, vp, vp, vp, sz, P(i32), cf, ci, ci, cd, cd, ci, ci, ci, ci, vp, vp, vp, vp, sz, vp]),
}
# include_ext/vistaf_centreline.h: the centreline read-out, two plain functions, the same pattern (tests/test_centrelines.py holds it
# against that header), and csrc/test_hooks_centreline.h: which storage tier a box takes
CENTRELINE_SIGNATURES = {
    "vistaf_centreline_workspace_bytes": (ci, [ci, ci, ci, ci, P(sz)]),
    "vistaf_centreline_measure": (ci, [vp, vp, vp, vp, vp, ci, ci, ci, ci, ci, ci, vp, vp, vp, vp, vp, vp, sz, vp]),
}
CENTRELINE_TEST_SIGNATURES = {
    "vistaf_ftp_test_centreline_tier": (ci, [ci, ci]),
}
# include_ext/vistaf_lobes.h: the lobe read-out, two plain functions, the same pattern (tests/test_lobes.py holds it against that header), and
# csrc/test_hooks_lobes.h: which storage tier a box takes
LOBES_SIGNATURES = {
    "vistaf_lobes_workspace_bytes": (ci, [ci, ci, ci, ci, P(sz)]),
    "vistaf_lobes_measure": (ci, [vp, vp, vp, vp, vp, ci, ci, ci, ci, ci, cd, cd, cd, vp, vp, vp, vp, vp, vp, vp, vp, sz, vp]),
}
LOBES_TEST_SIGNATURES = {
    "vistaf_ftp_test_lobes_tier": (ci, [ci, ci]),
}
# csrc/test_hooks_post.h: the back end of a predict (smoothing, sign flip, hole glue, composition and mm curve, blob filter, force tail, output
# copy) on planes of the caller (tests/test_post_direct.py holds the table against that header)
POST_SIGNATURES = {
    "vistaf_ftp_test_smooth_reliable": (ci, [vp, vp, vp, cd, vp, ci, ci, ci, ci, vp]),
    "vistaf_ftp_test_core_flip": (ci, [vp, vp, vp, ci, ci, vp]),
    "vistaf_ftp_test_hole_candidates": (ci, [vp, vp, vp, ci, cf, cf, vp, ci, ci, ci, vp]),
    "vistaf_ftp_test_hole_tmp": (ci, [vp, vp, vp, vp, vp, ci, ci, vp]),
    "vistaf_ftp_test_hole_zin": (ci, [vp, vp, ci, ci, vp]),
    "vistaf_ftp_test_hole_merge": (ci, [vp, vp, vp, vp, vp, ci, ci, vp]),
    "vistaf_ftp_test_height_finish": (ci, [vp, vp, vp, vp, vp, vp, cf, ci, cd, ci, cd, cd, cd, ci, vp, vp, vp, vp, ci, ci, ci, ci, vp]),
    "vistaf_ftp_test_to_mm": (ci, [vp, vp, ci, cd, cd, cd, ci, vp, vp, vp, ci, ci, vp]),
    "vistaf_ftp_test_tail": (ci, [vp, vp, vp, vp, cd, cd, cd, ci, cd, cd, cd, vp, ci, vp, ci, ci, ci, vp]),
    "vistaf_ftp_test_backend": (ci, [vp, vp, vp, vp, vp, vp, vp, cd, cd, cd, cd, cd, ci, cd, cd, cd, vp, vp, vp, vp, ci, vp, vp, ci, ci, ci, ci, vp]),
    "vistaf_ftp_test_backend_fits": (ci, [ci, ci]),
    "vistaf_ftp_test_frame_records": (ci, [vp, vp, vp, vp, vp, vp, vp, ci, vp, ci, vp]),
}
# every table beside SIGNATURES, a sixth read-out's included: load() applies what is listed here
EXTENSION_SIGNATURES = [MASK_CHAIN_SIGNATURES, DFT_STAGED_SIGNATURES, GAUSS_STRIP_SIGNATURES, FIT_WINDOW_SIGNATURES, OUTLINE_SIGNATURES, TEXTURE_SIGNATURES,
                        MATCH_SIGNATURES, CENTRELINE_SIGNATURES, CENTRELINE_TEST_SIGNATURES, LOBES_SIGNATURES, LOBES_TEST_SIGNATURES, POST_SIGNATURES]
# the names of each group, for the tests that hold them against the headers
(EXPORTS, ALIGN_EXPORTS, TEST_EXPORTS, TEMP_EXPORTS, TEMPMODEL_EXPORTS, TSENSOR_EXPORTS, TRACK_EXPORTS, SHAPE_EXPORTS, TAXEL_EXPORTS, THERMAL_EXPORTS,
 TEMPORAL_EXPORTS, CLOUD_EXPORTS, MOTION_EXPORTS, PRESSURE_EXPORTS) = (list(group) for group in SIGNATURES.values())

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
    for group in list(SIGNATURES.values()) + EXTENSION_SIGNATURES:
        for name, (restype, argtypes) in group.items():
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = restype, argtypes
    _lib = lib
    return lib


def check(rc: int):
    if rc != 0:
        msg = load().vistaf_ftp_last_error().decode("utf-8", "replace")
        if rc == -1:
            raise ValueError(msg)
        raise RuntimeError(f"vistaf_ftp error {rc}: {msg}")
