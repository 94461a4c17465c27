"""Result writers with the reference's file schemas, host side only.

* `result_record` / `write_result_json` / `write_result_csv` -- `Code/force_sensor.py:242-295`: the dict written to
  `result.json` (same keys, same order, same nesting of `force_model`) and the one-row `result.csv`.
* `height_map_bundle` / `export_heightmap_files` -- `Code/shape_ftp.py:260-310` and the call at `:1875-1932`:
  `height_map_crop.npy`, `height_map_full.npy`, optional CSVs and `height_map_bundle.npz` with the keys
  `height_crop`, `height_full`, seven `crop_*` and seven `full_*` boolean masks and ten `meta_*` int32 scalars, so the
  bundles the reference stored can be diffed key by key against the ones written from the GPU path.

* `multimodal_summary` / `write_multimodal_summary` -- `Code/multimodal_sensor.py:592-650` with its metric extractors (:214-280): the
  `multimodal_summary.json` of a combined force + temperature session (same keys, order and nesting).

* `tracks_table` / `write_tracks_csv` -- the contact tracker's table (`FtpSensor.track`, `tracks.ContactTracker`) as row dicts and as
  `tracks.csv`; an extension as the contacts table.

* `shapes_table` / `write_shapes_csv` -- the per-contact shape table (`FtpSensor.shapes`, `shapes.ContactShapes`) as row dicts and as
  `shapes.csv`; an extension as the contacts table.

* `taxels_table` / `write_taxels_csv` / `taxel_frame_record` -- the taxel read-out (`FtpSensor.taxels`, `taxels.TaxelReadout`) as row dicts,
  as `taxels.csv`, and the frame row as a dict; an extension as the contacts table.

* `thermal_table` / `write_thermal_csv` / `thermal_frame_record` -- the thermal read-out (`FtpSensor.thermal`, `thermal.ThermalReadout`) as row
  dicts, as `thermal.csv`, and the frame row as a dict; an extension as the contacts table.

* `temporal_table` / `write_temporal_csv` / `temporal_frame_record` -- the frame rows of the temporal read-out (`FtpSensor.temporal`,
  `temporal.TemporalReadout`) as row dicts, as `temporal.csv`, and one row as a dict; an extension as the contacts table.

* `cloud_frame_record` / `write_cloud_ply` -- the frame row of the point-cloud read-out (`FtpSensor.cloud`, `cloud.CloudReadout`) as a dict, and
  its points as a binary little-endian PLY file; an extension as the contacts table.

* `contacts_table` / `write_contacts_csv` / `contacts_record` -- the per-contact table of `FtpSensor.contacts` as row dicts, as
  `contacts.csv`, and as a `{"contact_count", "contacts"}` block for a JSON of the caller's own.  An extension with no reference schema:
  it is never merged into result.json / result.csv / multimodal_summary.json, which keep the reference's keys.

These functions take NumPy arrays (what `FtpSensor.predict` / `FtpSensor.masks` return); nothing here touches the GPU.
"""
from __future__ import annotations

import csv
import json
import math
import os
from typing import Any, Dict, Mapping, Optional, Sequence, Tuple

import numpy as np

CROP_MASK_KEYS = ("roi_eroded", "reliable", "output_reliable", "circ_mask", "contact_kept_by_depth", "hole_candidates",
                  "contact_dilated")                                                    # shape_ftp.py:1898-1906, in that order
RESULT_CSV_FIELDS = ("reference_path", "deformed_path", "volume_cm3", "force_N", "contact_area_mm2", "max_depth_mm", "mm_per_px",
                     "estimated_grating_period_px", "ftp_output_dir", "force_model_type")   # force_sensor.py:269-280
CONTACT_FIELDS = ("pixels", "contact_pixels", "contact_area_mm2", "volume_cm3", "max_depth_mm", "argmax_index", "centroid_x", "centroid_y",
                  "force_N", "bbox_x0", "bbox_y0", "bbox_x1", "bbox_y1")                  # VISTAF_CONTACT_* order (include/vistaf_ftp.h)
CONTACT_INT_FIELDS = ("pixels", "contact_pixels", "argmax_index", "bbox_x0", "bbox_y0", "bbox_x1", "bbox_y1")
CONTACTS_CSV_FIELDS = ("frame", "contact") + CONTACT_FIELDS
TRACK_FIELDS = ("track_id", "age_frames", "parent_row", "events", "overlap_px", "dx", "dy", "dforce_N", "dvolume_cm3",
                "origin_track_id")                                                        # VISTAF_TRACK_* order (include/vistaf_track.h)
TRACK_INT_FIELDS = ("track_id", "age_frames", "parent_row", "events", "overlap_px", "origin_track_id")
TRACKS_CSV_FIELDS = ("frame", "contact") + TRACK_FIELDS
SHAPE_FIELDS = ("contact_pixels", "boundary_pixels", "footprint_cx", "footprint_cy", "major_axis_mm", "minor_axis_mm", "orientation_rad",
                "fit_pixels", "fit_status", "apex_x", "apex_y", "apex_depth_mm", "curvature_1_per_mm", "curvature_2_per_mm",
                "curvature_axis_rad", "radius_1_mm", "radius_2_mm", "fit_rms_mm")          # VISTAF_SHAPE_* order (include/vistaf_shape.h)
SHAPE_INT_FIELDS = ("contact_pixels", "boundary_pixels", "fit_pixels", "fit_status")
SHAPES_CSV_FIELDS = ("frame", "contact") + SHAPE_FIELDS
OUTLINE_FIELDS = ("pixels", "pieces", "holes", "edges", "edges_all", "perimeter_mm", "enclosed_pixels", "corners", "corners_written", "hull_vertices",
                  "hull_area_mm2", "solidity", "max_feret_mm", "max_feret_angle_rad", "min_feret_mm", "box_cx", "box_cy", "box_length_mm",
                  "box_width_mm", "box_angle_rad")                                       # VISTAF_OUTLINE_* order (include_ext/vistaf_outline.h)
OUTLINE_INT_FIELDS = ("pixels", "pieces", "holes", "edges", "edges_all", "corners", "corners_written", "hull_vertices")
OUTLINES_CSV_FIELDS = ("frame", "contact") + OUTLINE_FIELDS
TEXTURE_FIELDS = ("eval_pixels", "form_status", "form_c0", "form_c1", "form_c2", "form_c3", "form_c4", "form_c5", "sa_mm", "sq_mm", "ssk", "sku",
                  "sp_mm", "sv_mm", "sz_mm", "sp_pixel", "sv_pixel", "grad_pixels", "sdq", "sdr", "grad_dir_x", "grad_dir_y", "coherence",
                  "acf_valid_lags", "lobe_lags", "lobe_status", "sal_mm", "sal_lag_x", "sal_lag_y", "rmax_mm", "str", "pitch_mm", "pitch_acf",
                  "profile_samples")                                                     # VISTAF_TEXTURE_* order (include_ext/vistaf_texture.h)
TEXTURE_INT_FIELDS = ("eval_pixels", "form_status", "sp_pixel", "sv_pixel", "grad_pixels", "acf_valid_lags", "lobe_lags", "lobe_status", "sal_lag_x",
                      "sal_lag_y", "profile_samples")                                    # -1 for NaN: what a status leaves out
TEXTURES_CSV_FIELDS = ("frame", "contact") + TEXTURE_FIELDS
MATCH_FIELDS = ("status", "flags", "label", "template", "class", "rotation", "shift_x", "shift_y", "score", "angle_rad", "x_px", "y_px", "offset_x_mm",
                "offset_y_mm", "second_class", "second_score", "margin", "rot_contrast", "scale", "base_mm", "resid_rms_mm", "support_pixels",
                "valid_shifts")                                                          # VISTAF_MATCH_* order (include_ext/vistaf_match.h)
MATCH_INT_FIELDS = ("status", "flags", "label", "template", "class", "rotation", "shift_x", "shift_y", "second_class", "support_pixels",
                    "valid_shifts")                                                      # -1 for NaN: what a status leaves out
MATCHES_CSV_FIELDS = ("frame", "contact") + MATCH_FIELDS
CENTRELINE_FIELDS = ("pixels", "skeleton_pixels", "thinning_passes", "end_pixels", "branch_pixels", "stations", "stations_written", "status", "a_x",
                     "a_y", "b_x", "b_y", "path_length_mm", "length_mm", "chord_mm", "tortuosity", "sagitta_mm", "sagitta_station",
                     "interior_stations", "width_mean_mm", "width_min_mm", "width_min_station", "width_max_mm", "width_max_station", "width_seed_mm",
                     "elongation", "a_tx", "a_ty", "b_tx", "b_ty", "a_at_border", "b_at_border", "depth_mean_mm", "depth_a_mm", "depth_b_mm",
                     "depth_peak_mm", "depth_peak_station")                              # VISTAF_CENTRELINE_* order (include_ext/vistaf_centreline.h)
CENTRELINE_INT_FIELDS = ("pixels", "skeleton_pixels", "thinning_passes", "end_pixels", "branch_pixels", "stations", "stations_written", "status",
                         "a_x", "a_y", "b_x", "b_y", "sagitta_station", "interior_stations", "width_min_station", "width_max_station",
                         "a_at_border", "b_at_border", "depth_peak_station")             # -1 for NaN: what a row without pixels, or without depth, leaves out
CENTRELINES_CSV_FIELDS = ("frame", "contact") + CENTRELINE_FIELDS
LOBE_FIELDS = ("x", "y", "depth_mm", "prominence_mm", "saddle_x", "saddle_y", "saddle_depth_mm", "neighbour", "pixels", "contact_pixels", "area_mm2",
               "volume_cm3", "centroid_x", "centroid_y", "force_share_N", "basins")       # VISTAF_LOBE_* order (include_ext/vistaf_lobes.h)
LOBE_INT_FIELDS = ("x", "y", "saddle_x", "saddle_y", "neighbour", "pixels", "contact_pixels", "basins")   # -1 for NaN: a peak without a saddle
LOBE_ROW_FIELDS = ("pixels", "raw_maxima", "peaks", "peaks_written", "status", "threshold_mm", "separation_mm", "deepest_saddle_mm",
                   "next_prominence_mm")                                                 # VISTAF_LOBEROW_* order
LOBE_ROW_INT_FIELDS = ("pixels", "raw_maxima", "peaks", "peaks_written", "status")
LOBES_CSV_FIELDS = ("frame", "contact", "lobe") + LOBE_FIELDS
TAXEL_FIELDS = ("contact_pixels", "contact_area_mm2", "volume_cm3", "mean_depth_mm", "max_depth_mm", "argmax_index", "centroid_x", "centroid_y",
                "force_N", "pressure_kPa")                                                # VISTAF_TAXEL_* order (include/vistaf_taxel.h)
TAXEL_INT_FIELDS = ("contact_pixels", "argmax_index")                                     # argmax_index is -1 for a taxel without contact
TAXELS_CSV_FIELDS = ("frame", "taxel") + TAXEL_FIELDS
TAXEL_FRAME_FIELDS = ("active_taxels", "volume_cm3", "force_N", "cop_x", "cop_y", "moment_x_Nmm", "moment_y_Nmm", "peak_taxel")   # VISTAF_TAXELFRAME_*
TAXEL_FRAME_INT_FIELDS = ("active_taxels", "peak_taxel")                                  # peak_taxel is -1 without an active taxel
THERMAL_FIELDS = ("contact_pixels", "valid_pixels", "coverage", "mean_C", "weighted_mean_C", "min_C", "max_C", "std_C", "peak_temp_C",
                  "surround_pixels", "surround_mean_C", "contrast_C")                     # VISTAF_THERMAL_* order (include/vistaf_thermal.h)
THERMAL_INT_FIELDS = ("contact_pixels", "valid_pixels", "surround_pixels")
THERMAL_CSV_FIELDS = ("frame", "contact") + THERMAL_FIELDS
THERMAL_FRAME_FIELDS = ("registered_pixels", "skin_mean_C", "contact_pixels", "contact_mean_C", "contrast_C", "hottest_contact",
                        "coldest_contact")                                                # VISTAF_THERMALFRAME_*
TEMPORAL_FIELDS = ("touch_pixels", "onset_pixels", "release_pixels", "loading_pixels", "unloading_pixels", "filtered_volume_cm3", "dvolume_cm3_per_s",
                   "max_filtered_mm", "argmax_index", "max_rate_mm_per_s", "max_rate_index", "min_rate_mm_per_s", "min_rate_index",
                   "longest_dwell_frames", "events", "gap_frames")                          # VISTAF_TEMPORAL_* order (include/vistaf_temporal.h)
TEMPORAL_INT_FIELDS = ("touch_pixels", "onset_pixels", "release_pixels", "loading_pixels", "unloading_pixels", "argmax_index", "max_rate_index",
                       "min_rate_index", "longest_dwell_frames", "events", "gap_frames")   # -1 for NaN: no touching pixel, or a skipped frame
TEMPORAL_CSV_FIELDS = ("frame", "skipped") + TEMPORAL_FIELDS
CLOUD_POINT_FIELDS = ("x", "y", "z", "nx", "ny", "nz", "curvature", "gaussian_curvature")   # VISTAF_CLOUD_* order (include/vistaf_cloud.h); the PLY properties
CLOUD_FRAME_FIELDS = ("surface_pixels", "points", "points_written", "projected_area_mm2", "surface_area_mm2", "mean_normal_x", "mean_normal_y",
                      "mean_normal_z", "tilt_deg", "max_slope_deg", "max_slope_index")      # VISTAF_CLOUDFRAME_* order; field 11 is reserved
CLOUD_FRAME_INT_FIELDS = ("surface_pixels", "points", "points_written", "max_slope_index")   # -1 for NaN: no surface pixel, or a skipped frame
MOTION_FIELDS = ("parent_row", "template_pixels", "status", "iterations", "tx_px", "ty_px", "theta_rad", "beta_mm", "tx_mm", "ty_mm", "centre_x",
                 "centre_y", "rms_before_mm", "rms_after_mm", "last_step_px", "se_tx_px", "se_ty_px", "se_theta_rad", "tx_minus_dx",
                 "ty_minus_dy")                                                          # VISTAF_MOTION_* order (include/vistaf_motion.h)
MOTION_INT_FIELDS = ("parent_row", "template_pixels", "status", "iterations")
MOTION_CSV_FIELDS = ("frame", "contact") + MOTION_FIELDS
MOTION_FRAME_FIELDS = ("registered", "max_slide_mm", "max_slide_row", "max_twist_rad", "max_twist_row", "mean_tx_mm", "mean_ty_mm",
                       "mean_rms_after_mm")                                              # VISTAF_MOTIONFRAME_*
PRESSURE_FIELDS = ("pixels", "force_model_N", "tensile_model_N", "force_N", "mean_kPa", "peak_kPa", "peak_index", "cop_x", "cop_y", "offset_x_mm",
                   "offset_y_mm", "peak_over_mean", "edge_share")                         # VISTAF_PRESSURE_* order (include/vistaf_pressure.h)
PRESSURE_INT_FIELDS = ("pixels", "peak_index")
PRESSURE_CSV_FIELDS = ("frame", "contact") + PRESSURE_FIELDS
PRESSURE_FRAME_FIELDS = ("contacts", "force_model_N", "tensile_model_N", "outside_model_N", "scale", "E_effective_MPa", "peak_kPa", "peak_index",
                         "peak_row", "cop_x", "cop_y", "status")                          # VISTAF_PRESSUREFRAME_* order
PRESSURE_FRAME_INT_FIELDS = ("contacts", "peak_index", "peak_row", "status")              # -1 for NaN: a frame whose status is not 0
MOTION_FRAME_INT_FIELDS = ("registered", "max_slide_row", "max_twist_row")               # -1 for NaN: no registered row, or a frame without contacts
THERMAL_FRAME_INT_FIELDS = ("registered_pixels", "contact_pixels", "hottest_contact", "coldest_contact")   # -1 for NaN: no contact has a mean


def _safe_float(x, default):
    """force_sensor.safe_float (:60-66): float(x) if finite else default."""
    try:
        v = float(x)
        return v if math.isfinite(v) else default
    except Exception:
        return default


def result_record(res: Mapping[str, Any], best_model: Mapping[str, Any], reference_path: str, deformed_path: str, output_dir: str,
                  ftp_output_dir: str, grating_pitch_mm: float = 2.0, depth_eps_mm: float = 0.01) -> Dict[str, Any]:
    """The dict `force_sensor.main` dumps to result.json (:242-262).  `res`: what `FtpSensor.predict` returned."""
    period = res.get("estimated_grating_period_px", None)
    return {
        "reference_path": reference_path,
        "deformed_path": deformed_path,
        "output_dir": output_dir,
        "ftp_output_dir": ftp_output_dir,
        "grating_pitch_mm": float(grating_pitch_mm),
        "depth_eps_mm": float(depth_eps_mm),
        "estimated_grating_period_px": None if period is None else _safe_float(period, float("nan")),
        "mm_per_px": float(res["mm_per_px"]),
        "volume_cm3": float(res["volume_cm3"]),
        "contact_area_mm2": float(res["contact_area_mm2"]),
        "max_depth_mm": float(res["max_depth_mm"]),
        "force_N": float(res["force_N"]),
        "force_model": {
            "type": best_model.get("type", ""),
            "params": best_model.get("params", {}),
            "equation": best_model.get("equation", ""),
            "rmse": best_model.get("rmse", None),
            "r2": best_model.get("r2", None),
        },
    }


def write_result_json(output_dir: str, record: Mapping[str, Any]) -> str:
    os.makedirs(output_dir, exist_ok=True)
    path = os.path.join(output_dir, "result.json")
    with open(path, "w", encoding="utf-8") as f:
        json.dump(record, f, indent=2)
    return path


def write_result_csv(output_dir: str, record: Mapping[str, Any]) -> str:
    os.makedirs(output_dir, exist_ok=True)
    path = os.path.join(output_dir, "result.csv")
    with open(path, "w", newline="", encoding="utf-8") as f:
        w = csv.DictWriter(f, fieldnames=list(RESULT_CSV_FIELDS))
        w.writeheader()
        row = {k: record[k] for k in RESULT_CSV_FIELDS if k != "force_model_type"}
        row["force_model_type"] = record["force_model"].get("type", "")
        w.writerow(row)
    return path


def _int_or_minus_one(v: float) -> int:
    return -1 if math.isnan(v) else int(v)


def _table(rows, count, fields, int_fields, error: str, *, with_contacts=None, skip_first=None, int_conv=int) -> list:
    """The row dicts of a per-contact table [B,K,>=len(fields)] (or [K,..] for one frame) with count [B]: `frame`, `contact` and `fields`,
    the `int_fields` through int_conv, for the first min(count, K) rows of every frame.  with_contacts: the contacts table of the same
    frames, whose [B,K] must agree.  skip_first: rows for whose first field it holds are left out.  ValueError(error) for other shapes."""
    t = np.asarray(rows, dtype=np.float64)
    n = np.atleast_1d(np.asarray(count)).astype(np.int64)
    if t.ndim == 2:
        t = t[None]
    ok = t.ndim == 3 and t.shape[2] >= len(fields) and t.shape[0] == n.shape[0]
    if with_contacts is not None:
        c = np.asarray(with_contacts, dtype=np.float64)
        if c.ndim == 2:
            c = c[None]
        ok = ok and c.ndim == 3 and c.shape[:2] == t.shape[:2]
    if not ok:
        raise ValueError(error)
    out = []
    for b in range(t.shape[0]):
        for k in range(min(max(int(n[b]), 0), t.shape[1])):
            if skip_first is not None and skip_first(t[b, k, 0]):
                continue
            row: Dict[str, Any] = {"frame": b, "contact": k}
            for i, name in enumerate(fields):
                row[name] = int_conv(t[b, k, i]) if name in int_fields else float(t[b, k, i])
            out.append(row)
    return out


def _write_csv(output_dir: str, filename: str, fieldnames, rows) -> str:
    """one line per row dict, floats with repr() (they read back to the same doubles)"""
    os.makedirs(output_dir, exist_ok=True)
    path = os.path.join(output_dir, filename)
    with open(path, "w", newline="", encoding="utf-8") as f:
        w = csv.DictWriter(f, fieldnames=list(fieldnames))
        w.writeheader()
        for row in rows:
            w.writerow({k: (repr(v) if isinstance(v, float) else v) for k, v in row.items()})
    return path


def _frame_record(row, fields, int_fields) -> Dict[str, Any]:
    """one frame row [>=len(fields)] as a dict of `fields`, the `int_fields` as ints (-1 for NaN)"""
    f = np.asarray(row, dtype=np.float64)
    if f.ndim != 1 or f.shape[0] < len(fields):
        raise ValueError(f"the frame row must be [>={len(fields)}]")
    return {name: (_int_or_minus_one(f[i]) if name in int_fields else float(f[i])) for i, name in enumerate(fields)}


def contacts_table(contacts, count) -> list:
    """Row dicts of the per-contact table: contacts [B,K,>=13] (or [K,>=13] for one frame) float64 as `FtpSensor.contacts` returns it, count
    [B] (or a scalar).  One dict per written contact, frames in order, contacts in the table's order (deepest first): `frame`, `contact`
    and CONTACT_FIELDS, the counts / indices / box as ints.  A frame with count > K contributes its K written rows (the table is
    truncated there, which `count` shows); NaN rows are skipped."""
    return _table(contacts, count, CONTACT_FIELDS, CONTACT_INT_FIELDS, "contacts must be [B,K,>=13] with count [B]")


def contacts_record(contacts, count) -> Dict[str, Any]:
    """{"contact_count": [per frame], "contacts": [row dicts]} for a JSON document of the caller's own (never result.json, whose schema is
    the reference's).  A NaN centroid (a contact without a pixel above depth_eps_mm) becomes null."""
    rows = contacts_table(contacts, count)
    for r in rows:
        for k, v in r.items():
            if isinstance(v, float) and not math.isfinite(v):
                r[k] = None
    return {"contact_count": [int(v) for v in np.atleast_1d(np.asarray(count))], "contacts": rows}


def write_contacts_csv(output_dir: str, contacts, count, filename: str = "contacts.csv") -> str:
    """contacts.csv: one line per written contact, columns CONTACTS_CSV_FIELDS, floats with repr() (they read back to the same doubles)."""
    return _write_csv(output_dir, filename, CONTACTS_CSV_FIELDS, contacts_table(contacts, count))


def tracks_table(tracks, contacts, count) -> list:
    """Row dicts of the contact tracker's table: tracks [B,K,>=10] (or [K,>=10] for one frame) float64 as `FtpSensor.track` returns it, with
    the contacts table [B,K,>=13] and count [B] of the same frames.  One dict per written contact, as `contacts_table`: `frame`, `contact`
    (the row in both tables) and TRACK_FIELDS, the ids / age / rows / bitmask / pixel count as ints; dx .. dvolume_cm3 are NaN at birth."""
    return _table(tracks, count, TRACK_FIELDS, TRACK_INT_FIELDS, "tracks must be [B,K,>=10] with contacts [B,K,>=13] and count [B]",
                  with_contacts=contacts)


def write_tracks_csv(output_dir: str, tracks, contacts, count, filename: str = "tracks.csv") -> str:
    """tracks.csv: one line per written contact, columns TRACKS_CSV_FIELDS, floats with repr(); lines match contacts.csv's one to one."""
    return _write_csv(output_dir, filename, TRACKS_CSV_FIELDS, tracks_table(tracks, contacts, count))


def shapes_table(shapes, contacts, count) -> list:
    """Row dicts of the per-contact shape table: shapes [B,K,>=18] (or [K,>=18] for one frame) float64 as `FtpSensor.shapes` returns it, with
    the contacts table [B,K,>=13] and count [B] of the same frames.  One dict per written contact, as `contacts_table`: `frame`, `contact`
    (the row in both tables) and SHAPE_FIELDS, the pixel counts and the fit status as ints; what a status leaves out is NaN."""
    return _table(shapes, count, SHAPE_FIELDS, SHAPE_INT_FIELDS, "shapes must be [B,K,>=18] with contacts [B,K,>=13] and count [B]",
                  with_contacts=contacts)


def write_shapes_csv(output_dir: str, shapes, contacts, count, filename: str = "shapes.csv") -> str:
    """shapes.csv: one line per written contact, columns SHAPES_CSV_FIELDS, floats with repr(); lines match contacts.csv's one to one."""
    return _write_csv(output_dir, filename, SHAPES_CSV_FIELDS, shapes_table(shapes, contacts, count))


def outlines_table(outlines, count) -> list:
    """Row dicts of the contact outline table: outlines [B,K,>=20] (or [K,>=20] for one frame) float64 as `FtpSensor.outlines` returns it,
    count [B].  One dict per written contact, as `contacts_table`: `frame`, `contact` and OUTLINE_FIELDS, the counts as ints; a row without
    a pixel has NaN where the header leaves NaN (enclosed_pixels among them, which therefore stays a float)."""
    return _table(outlines, count, OUTLINE_FIELDS, OUTLINE_INT_FIELDS, "outlines must be [B,K,>=20] with count [B]")


def write_outlines_csv(output_dir: str, outlines, count, filename: str = "outlines.csv") -> str:
    """outlines.csv: one line per written contact, columns OUTLINES_CSV_FIELDS, floats with repr(); lines match contacts.csv's one to one."""
    return _write_csv(output_dir, filename, OUTLINES_CSV_FIELDS, outlines_table(outlines, count))


def outline_frame_record(outlines, vertices, offsets, count) -> Dict[str, Any]:
    """One frame's outlines for a JSON document of the caller's own: outlines [K,>=20], vertices [V,2], offsets [K+1], count (a scalar).
    {"contact_count", "outlines": the row dicts without `frame`, NaN as null, "polylines": per row the [[x, y], ...] list of its
    principal loop's corners, null for a row that was not written (corners_written < corners)}."""
    rows = outlines_table(np.asarray(outlines, dtype=np.float64), np.asarray([count]))
    v, o = np.asarray(vertices), np.asarray(offsets)
    if v.ndim != 2 or v.shape[1] != 2 or o.ndim != 1 or o.shape[0] != np.asarray(outlines).shape[0] + 1:
        raise ValueError("vertices must be [V,2] and offsets [K+1] for outlines [K,>=20]")
    lines = []
    for r in rows:
        r.pop("frame")
        k = r["contact"]
        lines.append([[int(x), int(y)] for x, y in v[o[k]:o[k + 1]]] if r["corners_written"] == r["corners"] else None)
        for name, val in r.items():
            if isinstance(val, float) and not math.isfinite(val):
                r[name] = None
    return {"contact_count": int(count), "outlines": rows, "polylines": lines}


def textures_table(textures, count) -> list:
    """Row dicts of the surface texture table: textures [B,K,>=34] (or [K,>=34] for one frame) float64 as `FtpSensor.textures` returns it,
    count [B].  One dict per written contact, as `contacts_table`: `frame`, `contact` and TEXTURE_FIELDS, the counts, statuses, pixel indices
    and lags as ints (-1 where the row's status leaves the field NaN); every other field a status leaves out is NaN."""
    return _table(textures, count, TEXTURE_FIELDS, TEXTURE_INT_FIELDS, "textures must be [B,K,>=34] with count [B]", int_conv=_int_or_minus_one)


def write_textures_csv(output_dir: str, textures, count, filename: str = "textures.csv") -> str:
    """textures.csv: one line per written contact, columns TEXTURES_CSV_FIELDS, floats with repr(); lines match contacts.csv's one to one."""
    return _write_csv(output_dir, filename, TEXTURES_CSV_FIELDS, textures_table(textures, count))


def texture_frame_record(textures, count, acf=None) -> Dict[str, Any]:
    """One frame's textures for a JSON document of the caller's own: textures [K,>=34], count (a scalar), optionally acf [K,2L+1,2L+1].
    {"contact_count", "textures": the row dicts without `frame`, NaN as null} and, with acf, "acf": per row its window as nested lists,
    invalid lags as null."""
    t = np.asarray(textures, dtype=np.float64)
    rows = textures_table(t, np.asarray([count]))
    for r in rows:
        r.pop("frame")
        for name, val in r.items():
            if isinstance(val, float) and not math.isfinite(val):
                r[name] = None
    rec: Dict[str, Any] = {"contact_count": int(count), "textures": rows}
    if acf is not None:
        a = np.asarray(acf, dtype=np.float64)
        if a.ndim != 3 or a.shape[0] != t.shape[0] or a.shape[1] != a.shape[2] or a.shape[1] % 2 != 1:
            raise ValueError("acf must be [K,2L+1,2L+1] for textures [K,>=34]")
        rec["acf"] = [[[None if not math.isfinite(v) else float(v) for v in line] for line in a[r["contact"]]] for r in rows]
    return rec


def matches_table(matches, count) -> list:
    """Row dicts of the indenter match table: matches [B,K,>=23] (or [K,>=23] for one frame) float64 as `FtpSensor.matches` returns it, count
    [B].  One dict per written contact, as `contacts_table`: `frame`, `contact` and MATCH_FIELDS, the status, flags, label, indices, shifts and
    counts as ints (-1 where the row's status leaves the field NaN; a withheld label and a missing second class are -1 in the table itself);
    every other field a status leaves out is NaN."""
    return _table(matches, count, MATCH_FIELDS, MATCH_INT_FIELDS, "matches must be [B,K,>=23] with count [B]", int_conv=_int_or_minus_one)


def write_matches_csv(output_dir: str, matches, count, filename: str = "matches.csv") -> str:
    """matches.csv: one line per written contact, columns MATCHES_CSV_FIELDS, floats with repr(); lines match contacts.csv's one to one."""
    return _write_csv(output_dir, filename, MATCHES_CSV_FIELDS, matches_table(matches, count))


def centrelines_table(centrelines, count) -> list:
    """Row dicts of the centreline table: centrelines [B,K,>=37] (or [K,>=37] for one frame) float64 as `FtpSensor.centrelines` returns it,
    count [B].  One dict per written contact, as `contacts_table`: `frame`, `contact` and CENTRELINE_FIELDS, the counts, status, end pixels,
    station numbers and border flags as ints (-1 where the header leaves the field NaN); every other field it leaves out is NaN."""
    return _table(centrelines, count, CENTRELINE_FIELDS, CENTRELINE_INT_FIELDS, "centrelines must be [B,K,>=37] with count [B]", int_conv=_int_or_minus_one)


def write_centrelines_csv(output_dir: str, centrelines, count, filename: str = "centrelines.csv") -> str:
    """centrelines.csv: one line per written contact, columns CENTRELINES_CSV_FIELDS, floats with repr(); lines match contacts.csv's one to one."""
    return _write_csv(output_dir, filename, CENTRELINES_CSV_FIELDS, centrelines_table(centrelines, count))


def centreline_frame_record(centrelines, stations, station_d2, offsets, count) -> Dict[str, Any]:
    """One frame's centrelines for a JSON document of the caller's own: centrelines [K,>=37], stations [V,2], station_d2 [V], offsets [K+1],
    count (a scalar).  {"contact_count", "centrelines": the row dicts without `frame`, NaN as null, "stations": per row the [[x, y], ...]
    list of its axis path from end A to end B, null for a row that was not written (stations_written < stations), "d2": per row the
    squared distances to the rim that go with them}."""
    rows = centrelines_table(np.asarray(centrelines, dtype=np.float64), np.asarray([count]))
    v, d, o = np.asarray(stations), np.asarray(station_d2), np.asarray(offsets)
    if v.ndim != 2 or v.shape[1] != 2 or d.ndim != 1 or d.shape[0] != v.shape[0] or o.ndim != 1 or o.shape[0] != np.asarray(centrelines).shape[0] + 1:
        raise ValueError("stations must be [V,2], station_d2 [V] and offsets [K+1] for centrelines [K,>=37]")
    lines, widths = [], []
    for r in rows:
        r.pop("frame")
        k = r["contact"]
        whole = r["stations_written"] == r["stations"]
        lines.append([[int(x), int(y)] for x, y in v[o[k]:o[k + 1]]] if whole else None)
        widths.append([int(q) for q in d[o[k]:o[k + 1]]] if whole else None)
        for name, val in r.items():
            if isinstance(val, float) and not math.isfinite(val):
                r[name] = None
    return {"contact_count": int(count), "centrelines": rows, "stations": lines, "d2": widths}


def lobes_table(lobes, lobe_rows, count) -> list:
    """Row dicts of the lobe read-out: lobes [B,K,L,>=16] and lobe_rows [B,K,>=9] (or [K,L,..] and [K,..] for one frame) float64 as
    `FtpSensor.lobes` returns them, count [B].  One dict per written lobe (the first peaks_written records of every row in use), frames,
    contacts and lobes in order: `frame`, `contact`, `lobe` and LOBE_FIELDS, the pixels, counts and the neighbour as ints (-1 where the
    header leaves the field NaN)."""
    t, r = np.asarray(lobes, dtype=np.float64), np.asarray(lobe_rows, dtype=np.float64)
    n = np.atleast_1d(np.asarray(count)).astype(np.int64)
    if t.ndim == 3 and r.ndim == 2:
        t, r = t[None], r[None]
    if t.ndim != 4 or r.ndim != 3 or t.shape[:2] != r.shape[:2] or t.shape[3] < len(LOBE_FIELDS) or r.shape[2] < len(LOBE_ROW_FIELDS) or t.shape[0] != n.shape[0]:
        raise ValueError("lobes must be [B,K,L,>=16] with lobe_rows [B,K,>=9] and count [B]")
    out = []
    for b in range(t.shape[0]):
        for k in range(min(max(int(n[b]), 0), t.shape[1])):
            for j in range(min(_int_or_minus_one(r[b, k, LOBE_ROW_FIELDS.index("peaks_written")]), t.shape[2])):
                row: Dict[str, Any] = {"frame": b, "contact": k, "lobe": j}
                for i, name in enumerate(LOBE_FIELDS):
                    row[name] = _int_or_minus_one(t[b, k, j, i]) if name in LOBE_INT_FIELDS else float(t[b, k, j, i])
                out.append(row)
    return out


def write_lobes_csv(output_dir: str, lobes, lobe_rows, count, filename: str = "lobes.csv") -> str:
    """lobes.csv: one line per written lobe, columns LOBES_CSV_FIELDS, floats with repr() (they read back to the same doubles)."""
    return _write_csv(output_dir, filename, LOBES_CSV_FIELDS, lobes_table(lobes, lobe_rows, count))


def lobe_frame_record(lobes, lobe_rows, count, split_contacts=None, split_count=None, split_parent=None) -> Dict[str, Any]:
    """One frame's lobes for a JSON document of the caller's own: lobes [K,L,>=16], lobe_rows [K,>=9], count (a scalar) and, if given, the
    split table [K,>=13] with its count and parents [K,2].  {"contact_count", "lobes": per row in use the list of its written lobes as dicts
    of LOBE_FIELDS, "lobe_rows": per row in use a dict of LOBE_ROW_FIELDS} and, with the split table, "split_count" and "split_contacts":
    the row dicts of `contacts_table` without `frame`, each with `parent` = [row, lobe].  NaN becomes null."""
    t, r = np.asarray(lobes, dtype=np.float64), np.asarray(lobe_rows, dtype=np.float64)
    if t.ndim != 3 or r.ndim != 2:
        raise ValueError("lobes must be [K,L,>=16] with lobe_rows [K,>=9]")

    def clean(d):
        return {k: (None if isinstance(v, float) and not math.isfinite(v) else v) for k, v in d.items()}
    used = min(max(int(count), 0), t.shape[0])
    per_row = [[] for _ in range(used)]
    for row in lobes_table(t, r, np.asarray([count])):
        row.pop("frame")
        per_row[row.pop("contact")].append(clean(row))
    rec: Dict[str, Any] = {"contact_count": int(count), "lobes": per_row,
                           "lobe_rows": [clean(_frame_record(r[k], LOBE_ROW_FIELDS, LOBE_ROW_INT_FIELDS)) for k in range(used)]}
    if split_contacts is not None:
        par = np.asarray(split_parent)
        rows = contacts_table(np.asarray(split_contacts, dtype=np.float64), np.asarray([split_count]))
        for row in rows:
            row.pop("frame")
            row["parent"] = [int(v) for v in par[row["contact"]]]
        rec["split_count"], rec["split_contacts"] = int(split_count), [clean(row) for row in rows]
    return rec


def match_frame_record(matches, count, scores=None) -> Dict[str, Any]:
    """One frame's matches for a JSON document of the caller's own: matches [K,>=23], count (a scalar), optionally scores [K,T].
    {"contact_count", "matches": the row dicts without `frame`, NaN as null} and, with scores, "scores": per row the best score of every
    template, NaN as null."""
    t = np.asarray(matches, dtype=np.float64)
    rows = matches_table(t, np.asarray([count]))
    for r in rows:
        r.pop("frame")
        for name, val in r.items():
            if isinstance(val, float) and not math.isfinite(val):
                r[name] = None
    rec: Dict[str, Any] = {"contact_count": int(count), "matches": rows}
    if scores is not None:
        a = np.asarray(scores, dtype=np.float64)
        if a.ndim != 2 or a.shape[0] != t.shape[0]:
            raise ValueError("scores must be [K,T] for matches [K,>=23]")
        rec["scores"] = [[None if not math.isfinite(v) else float(v) for v in a[r["contact"]]] for r in rows]
    return rec


def taxels_table(taxels) -> list:
    """Row dicts of the taxel read-out: taxels [B,T,>=10] (or [T,>=10] for one frame) float64 as `FtpSensor.taxels` returns it.  One dict per
    frame and taxel, in that order: `frame`, `taxel` and TAXEL_FIELDS, the pixel count and the arg-max index as ints (-1: a taxel without
    contact has no arg-max).  A frame whose rows are NaN (its status was not 0) has no rows."""
    t = np.asarray(taxels, dtype=np.float64)
    if t.ndim == 2:
        t = t[None]
    if t.ndim != 3 or t.shape[2] < len(TAXEL_FIELDS):
        raise ValueError("taxels must be [B,T,>=10]")
    rows = []
    for b in range(t.shape[0]):
        if np.isnan(t[b, :, 0]).all():
            continue
        for k in range(t.shape[1]):
            row: Dict[str, Any] = {"frame": b, "taxel": k}
            for i, name in enumerate(TAXEL_FIELDS):
                row[name] = _int_or_minus_one(t[b, k, i]) if name in TAXEL_INT_FIELDS else float(t[b, k, i])
            rows.append(row)
    return rows


def write_taxels_csv(output_dir: str, taxels, filename: str = "taxels.csv") -> str:
    """taxels.csv: one line per frame and taxel, columns TAXELS_CSV_FIELDS, floats with repr()."""
    return _write_csv(output_dir, filename, TAXELS_CSV_FIELDS, taxels_table(taxels))


def taxel_frame_record(frame_row) -> Dict[str, Any]:
    """One frame row [>=8] of the taxel read-out as a dict of TAXEL_FRAME_FIELDS; active_taxels and peak_taxel as ints (-1 for NaN)."""
    return _frame_record(frame_row, TAXEL_FRAME_FIELDS, TAXEL_FRAME_INT_FIELDS)


def thermal_table(thermal, contacts, count) -> list:
    """Row dicts of the thermal read-out: thermal [B,K,>=12] (or [K,>=12] for one frame) float64 as `FtpSensor.thermal` returns it, with the
    contacts table [B,K,>=13] and count [B] of the same frames.  One dict per written contact, as `contacts_table`: `frame`, `contact` (the row
    in both tables) and THERMAL_FIELDS, the pixel counts as ints; what has no value is NaN.  A frame whose rows are NaN (its status was not
    0) has no rows."""
    return _table(thermal, count, THERMAL_FIELDS, THERMAL_INT_FIELDS, "thermal must be [B,K,>=12] with contacts [B,K,>=13] and count [B]",
                  with_contacts=contacts, skip_first=np.isnan)


def write_thermal_csv(output_dir: str, thermal, contacts, count, filename: str = "thermal.csv") -> str:
    """thermal.csv: one line per written contact, columns THERMAL_CSV_FIELDS, floats with repr(); lines match contacts.csv's one to one
    (but for frames whose status was not 0)."""
    return _write_csv(output_dir, filename, THERMAL_CSV_FIELDS, thermal_table(thermal, contacts, count))


def thermal_frame_record(frame_row) -> Dict[str, Any]:
    """One frame row [>=7] of the thermal read-out as a dict of THERMAL_FRAME_FIELDS; the pixel counts and the two rows as ints (-1 for NaN)."""
    return _frame_record(frame_row, THERMAL_FRAME_FIELDS, THERMAL_FRAME_INT_FIELDS)


def temporal_frame_record(frame_row) -> Dict[str, Any]:
    """One frame row [>=16] of the temporal read-out as a dict of TEMPORAL_FIELDS; counts, indices, dwell, events and gap as ints (-1 for NaN)."""
    return _frame_record(frame_row, TEMPORAL_FIELDS, TEMPORAL_INT_FIELDS)


def temporal_table(frames) -> list:
    """Row dicts of the temporal read-out: frames [B,>=16] (or [>=16] for one frame) float64 as `FtpSensor.temporal` returns it.  One dict per
    frame, skipped frames included: `frame`, `skipped` (1 for a frame whose status was not 0: its row is NaN but for gap_frames) and
    TEMPORAL_FIELDS as `temporal_frame_record` gives them."""
    t = np.asarray(frames, dtype=np.float64)
    if t.ndim == 1:
        t = t[None]
    if t.ndim != 2 or t.shape[1] < len(TEMPORAL_FIELDS):
        raise ValueError("frames must be [B,>=16]")
    rows = []
    for b in range(t.shape[0]):
        row: Dict[str, Any] = {"frame": b, "skipped": int(np.isnan(t[b, 0]))}
        row.update(temporal_frame_record(t[b]))
        rows.append(row)
    return rows


def write_temporal_csv(output_dir: str, frames, filename: str = "temporal.csv") -> str:
    """temporal.csv: one line per frame, columns TEMPORAL_CSV_FIELDS, floats with repr()."""
    return _write_csv(output_dir, filename, TEMPORAL_CSV_FIELDS, temporal_table(frames))


def cloud_frame_record(frame_row) -> Dict[str, Any]:
    """One frame row [>=11] of the point-cloud read-out as a dict of CLOUD_FRAME_FIELDS; the counts and the index as ints (-1 for NaN)."""
    return _frame_record(frame_row, CLOUD_FRAME_FIELDS, CLOUD_FRAME_INT_FIELDS)


def write_cloud_ply(path: str, points, label=None) -> str:
    """points [N,8] float32 (the written part of the point-cloud read-out: `CloudReadout.trim`) as a binary little-endian PLY file: one vertex
    per point with the float properties CLOUD_POINT_FIELDS (x y z nx ny nz curvature gaussian_curvature) and, when label [N] is given, a
    char property `label` (the row of the point's contact, -1 for none).  Millimetres, the frame of include/vistaf_cloud.h."""
    pts = np.asarray(points)
    if pts.ndim != 2 or pts.shape[1] != len(CLOUD_POINT_FIELDS):
        raise ValueError("points must be [N,8]")
    fields = [(name, "<f4") for name in CLOUD_POINT_FIELDS]
    if label is not None:
        lab = np.asarray(label)
        if lab.shape != (pts.shape[0],):
            raise ValueError("label must be [N] for the N points")
        fields.append(("label", "i1"))
    body = np.empty(pts.shape[0], dtype=np.dtype(fields))
    for i, name in enumerate(CLOUD_POINT_FIELDS):
        body[name] = pts[:, i]
    if label is not None:
        body["label"] = lab
    header = ["ply", "format binary_little_endian 1.0", "comment millimetres; x right, y down, z away from the camera",
              "element vertex %d" % pts.shape[0]]
    header += ["property float %s" % name for name in CLOUD_POINT_FIELDS]
    if label is not None:
        header.append("property char label")
    header.append("end_header")
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "wb") as f:
        f.write(("\n".join(header) + "\n").encode("ascii"))
        f.write(body.tobytes())
    return path


def motion_table(motion, contacts, count) -> list:
    """Row dicts of the contact motion table: motion [B,K,>=20] (or [K,>=20] for one frame) float64 as `FtpSensor.motion` returns it, with
    the contacts table [B,K,>=13] and count [B] of the same frames.  One dict per written contact, as `tracks_table`: `frame`, `contact`
    (the row in both tables) and MOTION_FIELDS, the parent row, pixel count, status and iterations as ints; what a status leaves out is NaN."""
    return _table(motion, count, MOTION_FIELDS, MOTION_INT_FIELDS, "motion must be [B,K,>=20] with contacts [B,K,>=13] and count [B]",
                  with_contacts=contacts)


def write_motion_csv(output_dir: str, motion, contacts, count, filename: str = "motion.csv") -> str:
    """motion.csv: one line per written contact, columns MOTION_CSV_FIELDS, floats with repr(); lines match contacts.csv's one to one."""
    return _write_csv(output_dir, filename, MOTION_CSV_FIELDS, motion_table(motion, contacts, count))


def motion_frame_record(frame_row) -> Dict[str, Any]:
    """One frame row [>=8] of the motion read-out as a dict of MOTION_FRAME_FIELDS; the count and the two rows as ints (-1 for NaN)."""
    return _frame_record(frame_row, MOTION_FRAME_FIELDS, MOTION_FRAME_INT_FIELDS)


def pressure_table(rows, count) -> list:
    """Row dicts of the pressure table: rows [B,K,>=13] (or [K,>=13] for one frame) float64 as `FtpSensor.pressure` returns it, with count [B]
    of the same frames.  One dict per written contact, as `contacts_table`: `frame`, `contact` (the row in both tables) and PRESSURE_FIELDS,
    the pixel count and the peak's index as ints; a field whose divisor is 0 is NaN."""
    return _table(rows, count, PRESSURE_FIELDS, PRESSURE_INT_FIELDS, "rows must be [B,K,>=13] with count [B]",
                  skip_first=lambda v: not np.isfinite(v), int_conv=_int_or_minus_one)        # not finite: a frame whose status is not 0


def write_pressure_csv(output_dir: str, rows, count, filename: str = "pressure.csv") -> str:
    """pressure.csv: one line per written contact, columns PRESSURE_CSV_FIELDS, floats with repr(); lines match contacts.csv's one to one."""
    return _write_csv(output_dir, filename, PRESSURE_CSV_FIELDS, pressure_table(rows, count))


def pressure_frame_record(frame_row) -> Dict[str, Any]:
    """One frame row [>=12] of the pressure read-out as a dict of PRESSURE_FRAME_FIELDS; the count, the peak's index and row and the status
    as ints (-1 for NaN)."""
    return _frame_record(frame_row, PRESSURE_FRAME_FIELDS, PRESSURE_FRAME_INT_FIELDS)


def height_map_bundle(height_crop: np.ndarray, crop_masks: Mapping[str, np.ndarray], crop_box: Tuple[int, int, int, int],
                      full_shape: Tuple[int, int], circle_full: Tuple[int, int, int], circle_crop: Tuple[int, int, int]) -> Dict[str, np.ndarray]:
    """Arrays of `height_map_bundle.npz` (shape_ftp.py:292-309 with the arguments of :1895-1930).
    crop_box = (x1, y1, x2, y2) of the ROI crop in the full frame; full_shape = (H, W)."""
    x1, y1, x2, y2 = (int(v) for v in crop_box)
    H, W = (int(v) for v in full_shape)
    hc = np.asarray(height_crop).astype(np.float32)
    if hc.shape != (y2 - y1, x2 - x1):
        raise ValueError("height_crop does not match the crop box")
    missing = [k for k in CROP_MASK_KEYS if k not in crop_masks]
    if missing:
        raise ValueError(f"missing crop masks: {missing}")
    full = np.full((H, W), np.nan, np.float32)
    full[y1:y2, x1:x2] = hc
    bundle: Dict[str, np.ndarray] = {"height_crop": hc, "height_full": full}
    for k in CROP_MASK_KEYS:
        bundle[f"crop_{k}"] = np.asarray(crop_masks[k]).astype(bool)
    for k in CROP_MASK_KEYS:
        m = np.zeros((H, W), dtype=bool)
        m[y1:y2, x1:x2] = bundle[f"crop_{k}"]
        bundle[f"full_{k}"] = m
    meta = {
        "crop_x1": x1, "crop_y1": y1, "crop_x2": x2, "crop_y2": y2,
        "roi_center_x_full": circle_full[0], "roi_center_y_full": circle_full[1], "roi_radius_full": circle_full[2],
        "roi_center_x_crop": circle_crop[0], "roi_center_y_crop": circle_crop[1], "roi_radius_crop": circle_crop[2],
    }
    for k, v in meta.items():
        bundle[f"meta_{k}"] = np.asarray(np.int32(v))
    return bundle


def export_heightmap_files(output_dir: str, bundle: Mapping[str, np.ndarray], basename: str = "height_map", save_crop_csv: bool = True,
                           save_full_csv: bool = False) -> Dict[str, str]:
    """shape_ftp.export_heightmap_files (:260-310): <basename>_crop.npy, _full.npy, optional CSVs ("%.9g"), _bundle.npz."""
    os.makedirs(output_dir, exist_ok=True)
    paths = {"crop_npy": os.path.join(output_dir, f"{basename}_crop.npy"), "full_npy": os.path.join(output_dir, f"{basename}_full.npy"),
             "bundle_npz": os.path.join(output_dir, f"{basename}_bundle.npz")}
    np.save(paths["crop_npy"], bundle["height_crop"].astype(np.float32))
    np.save(paths["full_npy"], bundle["height_full"].astype(np.float32))
    if save_crop_csv:
        paths["crop_csv"] = os.path.join(output_dir, f"{basename}_crop.csv")
        np.savetxt(paths["crop_csv"], bundle["height_crop"].astype(np.float32), delimiter=",", fmt="%.9g")
    if save_full_csv:
        paths["full_csv"] = os.path.join(output_dir, f"{basename}_full.csv")
        np.savetxt(paths["full_csv"], bundle["height_full"].astype(np.float32), delimiter=",", fmt="%.9g")
    np.savez_compressed(paths["bundle_npz"], **{k: np.asarray(v) for k, v in bundle.items()})
    return paths


# ---- multimodal_summary.json (Code/multimodal_sensor.py:592-650) ------------------------------------------------------------------
def _nan_float(x) -> float:
    """multimodal_sensor.safe_float (:95-102): float(x) if finite else NaN"""
    return _safe_float(x, float("nan"))


def _phase_to_height_metrics(calib: Optional[Mapping[str, Any]]) -> Dict[str, Any]:
    """extract_phase_to_height_metrics (:214-227)"""
    if calib is None:
        return {}
    best = calib.get("best_model", {})
    return {"calibration_type": "phase_to_height", "model_type": best.get("type", "unknown"), "equation": best.get("equation", ""),
            "r2": _nan_float(best.get("r2", float("nan"))), "rmse": _nan_float(best.get("rmse", float("nan"))),
            "n_samples": int(best.get("n", 0)), "x_definition": calib.get("x_definition", "")}


def _height_to_force_metrics(calib: Optional[Mapping[str, Any]]) -> Dict[str, Any]:
    """extract_height_to_force_metrics (:229-243)"""
    if calib is None:
        return {}
    best = calib.get("best_model", {})
    return {"calibration_type": "height_to_force", "model_type": best.get("type", "unknown"), "equation": best.get("equation", ""),
            "r2": _nan_float(best.get("r2", float("nan"))), "rmse": _nan_float(best.get("rmse", float("nan"))),
            "n_fit": int(best.get("n_fit", 0)), "n_samples": int(best.get("n_samples", 0)),
            "volume_definition": calib.get("volume_definition", "")}


def _temp_model_metrics(calib: Optional[Mapping[str, Any]], model_name: str) -> Dict[str, Any]:
    """extract_temp_model_metrics (:245-280)"""
    if calib is None:
        return {}
    models = calib.get("models_final", {})
    if model_name not in models:
        return {}
    m = models[model_name]

    def block(d):
        return {"rmse_C": _nan_float(d.get("rmse_C", float("nan"))), "mae_C": _nan_float(d.get("mae_C", float("nan"))),
                "r2": _nan_float(d.get("r2", float("nan"))), "max_abs_err_C": _nan_float(d.get("max_abs_err_C", float("nan"))),
                "p95_abs_err_C": _nan_float(d.get("p95_abs_err_C", float("nan"))), "n": int(d.get("n", 0))}
    return {"model": model_name, "degree": int(m.get("degree", 0)), "equation": m.get("equation", ""),
            "frames": block(m.get("metrics_frames", {})), "means": block(m.get("metrics_means", {}))}


def temperature_statistics(temp_map_C, valid_mask) -> Dict[str, Any]:
    """mean / median / std / min / max of the final temperature map over its valid pixels (multimodal_sensor.py:558-567), in the key order
    of the summary's `temperature` block; NaN statistics when no pixel is valid."""
    t = np.asarray(temp_map_C)
    valid = np.asarray(valid_mask, dtype=bool)
    if np.any(valid):
        v = t[valid]
        st = {"mean_C": float(np.mean(v)), "median_C": float(np.median(v)), "std_C": float(np.std(v)), "min_C": float(np.min(v)),
              "max_C": float(np.max(v))}
    else:
        st = {k: float("nan") for k in ("mean_C", "median_C", "std_C", "min_C", "max_C")}
    st["valid_pixels"] = int(np.count_nonzero(valid))
    return st


def multimodal_summary(session_id: str, timestamp: str, reference_image: str, deformed_image: str, session_dir: str, force: Mapping[str, Any],
                       temperature: Mapping[str, Any], p2h_calib: Optional[Mapping[str, Any]], h2f_calib: Optional[Mapping[str, Any]],
                       color_calib: Optional[Mapping[str, Any]], black_calib: Optional[Mapping[str, Any]], force_subdir: str,
                       temp_subdir: str, combined_subdir: str) -> Dict[str, Any]:
    """The dict `multimodal_sensor.main` dumps to combined_outputs/multimodal_summary.json (:592-644).  `force`: what `FtpSensor.predict`
    returned (force_N, volume_cm3, contact_area_mm2, max_depth_mm, mm_per_px); `temperature`: `temperature_statistics(...)`; the four
    calibration dicts are the loaded calibration JSONs (None when a file is missing, as upstream's load_json_safe returns)."""
    return {
        "session_id": session_id,
        "timestamp": timestamp,
        "input_images": {"reference": reference_image, "deformed": deformed_image},
        "output_directory": session_dir,
        "sensor_readings": {
            "force": {"force_N": force["force_N"], "volume_cm3": force["volume_cm3"], "contact_area_mm2": force["contact_area_mm2"],
                      "max_depth_mm": force["max_depth_mm"], "scale_mm_per_px": force["mm_per_px"]},
            "temperature": {k: temperature[k] for k in ("mean_C", "median_C", "std_C", "min_C", "max_C", "valid_pixels")},
        },
        "calibration_performance": {
            "phase_to_height": _phase_to_height_metrics(p2h_calib),
            "height_to_force": _height_to_force_metrics(h2f_calib),
            "temperature_color_model": {k: _temp_model_metrics(color_calib, k) for k in ("heating", "cooling", "global")} if color_calib else {},
            "temperature_black_model": {k: _temp_model_metrics(black_calib, k) for k in ("heating", "cooling", "global")} if black_calib else {},
        },
        "file_paths": {"force_subdir": force_subdir, "temperature_subdir": temp_subdir, "combined_subdir": combined_subdir},
    }


def write_multimodal_summary(combined_subdir: str, summary: Mapping[str, Any]) -> str:
    os.makedirs(combined_subdir, exist_ok=True)
    path = os.path.join(combined_subdir, "multimodal_summary.json")
    with open(path, "w", encoding="utf-8") as f:
        json.dump(summary, f, indent=2)                      # :648-649
    return path
