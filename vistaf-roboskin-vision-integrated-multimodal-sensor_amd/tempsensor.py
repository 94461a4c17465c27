"""The temperature modality end to end on the GPU: BGR photograph -> final temperature map, source map and statistics.

Reference interface mirrored:
  * `temperature_sensor.main()` (Code/temperature_sensor.py:749-870): segmentation, feature planes, colour support, both regressors, inpaint /
    clamp, per-pixel fusion and the oriented smoothing, on the full frame -- `TempSensor.predict`
  * the statistics of the final map the combined summary reports (Code/multimodal_sensor.py:558-567) -- `map_statistics`, equal to
    `writers.temperature_statistics` to the last bit
backed by `vistaf_tsensor_*` of libvistaf_ftp.so (include/vistaf_tempsensor.h, which states the chain and the one inferred step: the wide
model runs over roi_eff).  Parity unpinned as the map stages are.  Saved artefacts (PNG overlays, .npy files) are not produced here.
"""
from __future__ import annotations

import ctypes
import dataclasses
from typing import Any, Dict, Optional, Tuple

import numpy as np
import torch

from . import _lib
from ._handle import Handle
from .tempmodel import TempModel
from .tempseg import (BLUR_KSIZE, COLOR_CHROMA_MIN, COLOR_GUARD_BAND, COLOR_SUPPORT_DILATE, COLOR_T_MAX, COLOR_T_MIN, FINAL_SMOOTH_SIGMA_ACROSS,
                      FINAL_SMOOTH_SIGMA_ALONG, FINAL_T_MAX, FINAL_T_MIN, OUTER_CIRCLE, SWITCH_MARGIN_C, TempSegConfig, roi_mask_from_circle)

STAT_KEYS = ("mean_C", "median_C", "std_C", "min_C", "max_C", "valid_pixels")     # writers.temperature_statistics, in order
MASK_KEYS = ("roi_eff", "sat", "dark", "light", "color_support")                   # planes of d_masks (VISTAF_TSENSOR_MASK_*)
WIDE_INPAINT_RADIUS, COLOR_INPAINT_RADIUS, COLOR_CLAMP_PAD = 7, 5, 5.0            # main() :835-845


@dataclasses.dataclass
class TempSensorConfig:
    """Every constant of the chain, defaults as shipped (include/vistaf_tempsensor.h)"""
    seg: TempSegConfig = dataclasses.field(default_factory=TempSegConfig)
    color_t_min: float = COLOR_T_MIN
    color_t_max: float = COLOR_T_MAX
    color_guard_band: float = COLOR_GUARD_BAND
    switch_margin_c: float = SWITCH_MARGIN_C
    final_t_min: float = FINAL_T_MIN
    final_t_max: float = FINAL_T_MAX
    blur_ksize: int = BLUR_KSIZE
    color_support_dilate: int = COLOR_SUPPORT_DILATE
    wide_inpaint_radius: int = WIDE_INPAINT_RADIUS
    color_inpaint_radius: int = COLOR_INPAINT_RADIUS
    color_chroma_min: float = COLOR_CHROMA_MIN
    color_clamp_pad: float = COLOR_CLAMP_PAD
    smooth_sigma_across: float = FINAL_SMOOTH_SIGMA_ACROSS
    smooth_sigma_along: float = FINAL_SMOOTH_SIGMA_ALONG

    def to_c(self) -> "_lib.CTSensorConfig":
        cc = _lib.CTSensorConfig()
        cc.seg = self.seg.to_c()
        cc.fuse = _lib.CTempFuseConfig(self.color_t_min, self.color_t_max, self.color_guard_band, self.switch_margin_c, self.final_t_min,
                                       self.final_t_max)
        for n in ("blur_ksize", "color_support_dilate", "wide_inpaint_radius", "color_inpaint_radius", "color_chroma_min", "color_clamp_pad",
                  "smooth_sigma_across", "smooth_sigma_along"):
            setattr(cc, n, getattr(self, n))
        return cc


def _stats_dict(v) -> Dict[str, Any]:
    st = {k: float(v[i]) for i, k in enumerate(STAT_KEYS[:5])}
    st["valid_pixels"] = int(v[5])
    return st


class _StatsWorkspace(Handle):
    """Workspace of vistaf_tsensor_map_statistics for one map size on one device"""
    _destroy = "vistaf_tsensor_stats_destroy"

    def __init__(self, H: int, W: int, device: torch.device):
        self._open(device, need_device=False)
        self.H, self.W = H, W
        self._call("vistaf_tsensor_stats_create", H, W, ctypes.byref(self._h))

    def run(self, m: torch.Tensor, valid: Optional[torch.Tensor]) -> Dict[str, Any]:
        out = (ctypes.c_double * _lib.TSENSOR_NSTATS)()
        self._call("vistaf_tsensor_map_statistics", self._h, m.data_ptr(), None if valid is None else valid.data_ptr(), None, out, self._stream())
        return _stats_dict(out)


_workspaces: Dict[Tuple[int, int, int], _StatsWorkspace] = {}


def map_statistics(temp_map_C, valid=None, device=None) -> Dict[str, Any]:
    """writers.temperature_statistics(temp_map_C, valid) on the GPU, equal to it to the last bit (see include/vistaf_tempsensor.h for the
    two stated exceptions): a float32 [H, W] map (NumPy or device tensor), `valid` a boolean / uint8 [H, W] mask or None for
    isfinite(map).  Returns {"mean_C", "median_C", "std_C", "min_C", "max_C", "valid_pixels"}."""
    m = temp_map_C if torch.is_tensor(temp_map_C) else torch.from_numpy(np.ascontiguousarray(np.asarray(temp_map_C)))
    if m.dtype != torch.float32 or m.dim() != 2 or m.shape[0] < 1 or m.shape[1] < 1:
        raise ValueError(f"map must be float32 [H, W] with H, W >= 1, got {m.dtype} {tuple(m.shape)}")
    dev = torch.device(device) if device is not None else (m.device if m.is_cuda else torch.device("cuda:0"))
    m = m.to(dev).contiguous()
    v = None
    if valid is not None:
        v = valid if torch.is_tensor(valid) else torch.from_numpy(np.ascontiguousarray(np.asarray(valid)))
        if tuple(v.shape) != tuple(m.shape):
            raise ValueError("valid mask shape does not match the map")
        v = (v.to(dev) != 0).to(torch.uint8).contiguous()
    H, W = (int(s) for s in m.shape)
    idx = dev.index if dev.index is not None else torch.cuda.current_device()
    ws = _workspaces.get((H, W, idx))
    if ws is None:
        ws = _workspaces[(H, W, idx)] = _StatsWorkspace(H, W, torch.device("cuda", idx))
    return ws.run(m, v)


class TempSensor(Handle):
    """One session of temperature_sensor.main() for H x W photographs: every buffer, workspace and the smoothing taps are allocated at
    construction (H a multiple of 16, both sides >= 64, as the segmentation needs); `predict` allocates nothing on the library side."""
    _destroy = "vistaf_tsensor_destroy"

    def __init__(self, wide_model: TempModel, color_model: TempModel, frame_shape, roi_full=None, config: Optional[TempSensorConfig] = None,
                 device="cuda:0"):
        self._open(device)
        if not isinstance(wide_model, TempModel) or not isinstance(color_model, TempModel):
            raise ValueError("TempSensor needs a wide and a colour TempModel")
        self.config = config or TempSensorConfig()
        self.H, self.W = (int(v) for v in tuple(frame_shape)[:2])
        self.wide_model, self.color_model = wide_model, color_model           # the session keeps their device handles
        if roi_full is None:
            roi_full = roi_mask_from_circle(self.H, self.W, *OUTER_CIRCLE)
        r = roi_full if torch.is_tensor(roi_full) else torch.from_numpy(np.ascontiguousarray(np.asarray(roi_full)))
        if tuple(r.shape) != (self.H, self.W):
            raise ValueError("roi_full shape does not match the frame")
        self.roi_full = (r.to(self.device) != 0).to(torch.uint8).contiguous()
        cc = self.config.to_c()
        wh, ch = wide_model._handle(self.device), color_model._handle(self.device)
        self._call("vistaf_tsensor_create", ctypes.byref(cc), self.H, self.W, wh, ch, ctypes.byref(self._h))

    def predict(self, image_bgr) -> Dict[str, Any]:
        """temperature_sensor.main() on one [H, W, 3] uint8 BGR photograph.  Returns "temperature_map_C" (float32, NaN outside the ROI),
        "source_map" (uint8: 0 wide, 255 colour, 128 blend), "wide_map_C" / "color_map_C" (the clamped maps before fusion), "masks"
        (roi_full, roi_eff, sat, dark, light, color_support), "dbg" (the segmentation record and the fusion counts) and "statistics"
        (writers.temperature_statistics of the final map over its finite pixels; ready for writers.multimodal_summary(temperature=...)).
        NumPy in gives NumPy out; a device tensor in gives device tensors out."""
        on_dev = torch.is_tensor(image_bgr) and image_bgr.is_cuda
        img = image_bgr if torch.is_tensor(image_bgr) else torch.from_numpy(np.ascontiguousarray(image_bgr))
        if img.dtype != torch.uint8 or img.dim() != 3 or img.shape[2] != 3 or tuple(img.shape[:2]) != (self.H, self.W):
            raise ValueError(f"image must be [{self.H},{self.W},3] uint8 (BGR)")
        img = img.to(self.device).contiguous()
        shp, dev = (self.H, self.W), self.device
        final = torch.empty(shp, dtype=torch.float32, device=dev)
        wide, color = torch.empty_like(final), torch.empty_like(final)
        source = torch.empty(shp, dtype=torch.uint8, device=dev)
        masks = torch.empty((_lib.TSENSOR_NMASKS,) + shp, dtype=torch.uint8, device=dev)
        info = (ctypes.c_double * _lib.TSENSOR_NINFO)()
        stats = (ctypes.c_double * _lib.TSENSOR_NSTATS)()
        self._call("vistaf_tsensor_predict", self._h, img.data_ptr(), self.roi_full.data_ptr(), final.data_ptr(), source.data_ptr(), wide.data_ptr(),
                   color.data_ptr(), masks.data_ptr(), info, None, stats, self._stream())
        n0 = _lib.TEMPSEG_NINFO
        dbg = {
            "peak_x": int(info[0]), "peak_y": int(info[1]), "phi0_rad": float(info[2]), "mean_gray_A": float(info[3]), "mean_gray_B": float(info[4]),
            "chosen": "A_is_dark" if info[5] else "B_is_dark", "roi_pixels": int(info[6]), "roi_eff_pixels": int(info[7]), "sat_pixels": int(info[8]),
            "dark_pixels": int(info[9]), "light_pixels": int(info[10]), "carrier_angle_rad": float(info[11]), "carrier_period_px": float(info[12]),
            "fusion": {"roi_pixels": int(info[n0]), "wide_ok_pixels": int(info[n0 + 1]), "color_ok_pixels": int(info[n0 + 2]),
                       "blend_pixels": int(info[n0 + 3])},
        }
        mk = {"roi_full": self.roi_full.bool()}
        mk.update({k: masks[i].bool() for i, k in enumerate(MASK_KEYS)})
        res = {"temperature_map_C": final, "source_map": source, "wide_map_C": wide, "color_map_C": color, "masks": mk}
        if not on_dev:
            res = {k: ({n: t.cpu().numpy() for n, t in v.items()} if isinstance(v, dict) else v.cpu().numpy()) for k, v in res.items()}
        res["dbg"] = dbg
        res["statistics"] = _stats_dict(stats)
        return res

    def map_statistics(self, temp_map_C, valid=None) -> Dict[str, Any]:
        """map_statistics on this session's device"""
        return map_statistics(temp_map_C, valid, device=self.device)
