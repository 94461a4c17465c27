"""MI355X-native (gfx950) implementation of the VISTAF image -> height-map -> force path.

Drop-in for the Fourier-Transform-Profilometry hot path of
rimelq/VISTAF-RoboSkin-Vision-Integrated-Multimodal-Sensor (Code/shape_ftp.py + the force tail of
Code/force_sensor.py).  All image arithmetic runs in hand-written HIP kernels behind the C ABI of
include/vistaf_ftp.h; this package is the thin Python host side.  There is no CPU fallback.
"""
from . import _lib
from .config import FtpConfig
from .ftp import (FtpSensor, SCALAR_NAMES, CONTACT_NAMES, depth_map_to_volume_cm3, estimate_mm_per_px, frame_layout, load_calibration,
                  load_force_calibration, predict, predict_force_from_volume)
from . import tracks
from .tracks import ContactTracker, TRACK_NAMES, TRACK_EVENTS
from . import shapes
from .shapes import ContactShapes, SHAPE_NAMES
from . import taxels
from .taxels import TaxelLayout, TaxelReadout, TAXEL_NAMES, TAXEL_FRAME_NAMES, grid_layout, polar_layout, from_map
from . import thermal
from .thermal import ThermalReadout, THERMAL_NAMES, THERMAL_FRAME_NAMES
from . import temporal
from .temporal import TemporalReadout, TEMPORAL_NAMES, TEMPORAL_EVENTS
from . import cloud
from .cloud import CloudReadout, CLOUD_POINT_NAMES, CLOUD_FRAME_NAMES
from . import motion
from .motion import ContactMotion, MOTION_NAMES, MOTION_FRAME_NAMES, MOTION_STATUS
from . import pressure
from .pressure import PressureReadout, PRESSURE_NAMES, PRESSURE_FRAME_NAMES
from . import outline
from .outline import OUTLINE_NAMES, contact_outlines
from . import texture
from .texture import TEXTURE_NAMES, TextureWorkspace, contact_textures
from . import match
from .match import MATCH_NAMES, MatchWorkspace, TemplateBank, contact_matches
from . import centreline
from .centreline import CENTRELINE_NAMES, CENTRELINE_STATUS, CentrelineWorkspace, contact_centrelines
from . import lobes
from .lobes import LOBE_NAMES, LOBE_ROW_NAMES, LOBE_STATUS, LobesWorkspace, contact_lobes
from . import synth
from . import parallel
from .align import FtpAligner, circle_from_3_points
from . import calibrate
from . import tempseg
from .tempseg import TempSegConfig, TempSegmenter, segment_dark_light_gratings_periodic_fft, compute_feature_planes, color_support_mask
from . import tempmodel
from .tempmodel import TempModel, predict_map_for_mask, predict_maps
from . import tempsensor
from .tempsensor import TempSensor, TempSensorConfig, map_statistics
from .writers import (contacts_record, contacts_table, write_contacts_csv, tracks_table, write_tracks_csv, shapes_table, write_shapes_csv, taxels_table, write_taxels_csv, taxel_frame_record, thermal_table, write_thermal_csv, thermal_frame_record, temporal_table, write_temporal_csv, temporal_frame_record, cloud_frame_record, write_cloud_ply, motion_table, write_motion_csv, motion_frame_record, pressure_table, write_pressure_csv, pressure_frame_record, outlines_table, write_outlines_csv, outline_frame_record, centrelines_table, write_centrelines_csv, centreline_frame_record, lobes_table, write_lobes_csv, lobe_frame_record, textures_table, write_textures_csv, texture_frame_record, matches_table, write_matches_csv, match_frame_record, export_heightmap_files, height_map_bundle, multimodal_summary, result_record, temperature_statistics,
                      write_multimodal_summary, write_result_csv, write_result_json)

__all__ = ["FtpConfig", "FtpSensor", "SCALAR_NAMES", "CONTACT_NAMES", "contacts_table", "contacts_record", "write_contacts_csv", "ContactTracker", "TRACK_NAMES", "TRACK_EVENTS", "tracks", "tracks_table", "write_tracks_csv", "ContactShapes", "SHAPE_NAMES", "shapes", "shapes_table", "write_shapes_csv", "taxels", "TaxelLayout", "TaxelReadout", "TAXEL_NAMES", "TAXEL_FRAME_NAMES", "grid_layout", "polar_layout", "from_map", "taxels_table", "write_taxels_csv", "taxel_frame_record", "thermal", "ThermalReadout", "THERMAL_NAMES", "THERMAL_FRAME_NAMES", "thermal_table", "write_thermal_csv", "thermal_frame_record", "temporal", "TemporalReadout", "TEMPORAL_NAMES", "TEMPORAL_EVENTS", "temporal_table", "write_temporal_csv", "temporal_frame_record", "cloud", "CloudReadout", "CLOUD_POINT_NAMES", "CLOUD_FRAME_NAMES", "cloud_frame_record", "write_cloud_ply", "motion", "ContactMotion", "MOTION_NAMES", "MOTION_FRAME_NAMES", "MOTION_STATUS", "motion_table", "write_motion_csv", "motion_frame_record", "pressure", "PressureReadout", "PRESSURE_NAMES", "PRESSURE_FRAME_NAMES", "pressure_table", "write_pressure_csv", "pressure_frame_record", "outline", "OUTLINE_NAMES", "contact_outlines", "outlines_table", "write_outlines_csv", "outline_frame_record", "centreline", "CENTRELINE_NAMES", "CENTRELINE_STATUS", "CentrelineWorkspace", "contact_centrelines", "centrelines_table", "write_centrelines_csv", "centreline_frame_record", "lobes", "LOBE_NAMES", "LOBE_ROW_NAMES", "LOBE_STATUS", "LobesWorkspace", "contact_lobes", "lobes_table", "write_lobes_csv", "lobe_frame_record", "texture", "TEXTURE_NAMES", "TextureWorkspace", "contact_textures", "textures_table", "write_textures_csv", "texture_frame_record", "match", "MATCH_NAMES", "TemplateBank", "MatchWorkspace", "contact_matches", "matches_table", "write_matches_csv", "match_frame_record", "depth_map_to_volume_cm3", "estimate_mm_per_px", "frame_layout", "load_calibration",
           "load_force_calibration", "predict", "predict_force_from_volume", "synth", "parallel", "FtpAligner", "circle_from_3_points", "calibrate", "_lib", "export_heightmap_files",
           "height_map_bundle", "result_record", "write_result_csv", "write_result_json", "multimodal_summary", "temperature_statistics",
           "write_multimodal_summary", "tempseg", "TempSegConfig", "TempSegmenter", "segment_dark_light_gratings_periodic_fft", "compute_feature_planes", "color_support_mask",
           "tempmodel", "TempModel", "predict_map_for_mask", "predict_maps", "tempsensor", "TempSensor", "TempSensorConfig", "map_statistics"]
