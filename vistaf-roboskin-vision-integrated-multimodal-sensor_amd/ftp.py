"""Host-side mirror of the reference's image -> height-map -> force interface, backed by the HIP library.

Reference interface mirrored (paths relative to the reference tree):
  * Code/shape_ftp.py:1428-2037  `main(reference_path, deformed_path, ..., return_results=True)` ->
    {"height_map_mm_crop", "roi_eroded_crop", "output_reliable_crop", "estimated_grating_period_px"}
  * Code/force_sensor.py:93-123  `depth_map_to_volume_cm3(height_map_mm, roi_mask, mm_per_px, depth_eps_mm)`
  * Code/force_sensor.py:149-167 `predict_force_from_volume(best_model, volume_cm3)`
  * Code/force_sensor.py:173-187 `estimate_mm_per_px(period)`
  * Code/shape_ftp.py:672-680 / force_sensor.py:142-147 calibration JSON loaders
`predict(image[, reference]) -> force_map` is the name BASELINE.json asks for; it does not exist
upstream and is defined here as shape_ftp.main's result dict plus the force tail of
Code/multimodal_sensor.py:388-419.

PyTorch is used only for device memory and streams; all image arithmetic runs in libvistaf_ftp.so.
"""
from __future__ import annotations

import ctypes
import json
import math
from typing import Any, Dict, Optional, Tuple

import numpy as np
import torch

from . import _lib
from ._handle import Handle, call, stream
from .config import FtpConfig

SCALAR_NAMES = [
    "volume_cm3", "contact_area_mm2", "max_depth_mm", "force_N", "argmax_depth_index", "estimated_grating_period_px",
    "mm_per_px", "min_height_unitless", "argmin_unitless_index", "reliable_count", "sign_flipped", "amp_threshold",
    "contact_threshold", "bg_median", "bad_pixels", "reserved",
]
# fields of a row of the per-contact table, in the order of the VISTAF_CONTACT_* indices (include/vistaf_ftp.h); 13..15 are reserved
CONTACT_NAMES = [
    "pixels", "contact_pixels", "contact_area_mm2", "volume_cm3", "max_depth_mm", "argmax_index", "centroid_x", "centroid_y", "force_N",
    "bbox_x0", "bbox_y0", "bbox_x1", "bbox_y1",
]


def load_calibration(json_path: str) -> Tuple[Dict[str, Any], bool]:
    """shape_ftp.load_calibration (Code/shape_ftp.py:672-680): (best_model, use_negated_height)."""
    with open(json_path, "r", encoding="utf-8") as f:
        cal = json.load(f)
    return cal["best_model"], bool(cal.get("use_negated_height_for_fit", True))


def load_force_calibration(path: str) -> Dict[str, Any]:
    """force_sensor.load_force_calibration (Code/force_sensor.py:142-147)."""
    with open(path, "r", encoding="utf-8") as f:
        data = json.load(f)
    if "best_model" not in data:
        raise ValueError("Invalid force calibration JSON: missing 'best_model'")
    return data


def _curve(model: Dict[str, Any], what: str) -> _lib.Curve:
    t = model["type"]
    p = model["params"]
    if t not in _lib.CURVE_TYPES:
        raise ValueError(f"Unknown model type in {what}: {t}")
    c = _lib.Curve()
    c.type = _lib.CURVE_TYPES[t]
    if t == "poly2":
        c.a, c.b, c.c = float(p["c2"]), float(p["c1"]), float(p["c0"])
    else:
        c.a = float(p["a"])
        c.b = float(p.get("b", 0.0))
        c.c = float(p.get("c", 0.0))
    return c


def estimate_mm_per_px(estimated_grating_period_px: Optional[float], grating_pitch_mm: float = 2.0) -> float:
    """force_sensor.estimate_mm_per_px (Code/force_sensor.py:173-187)."""
    if estimated_grating_period_px is None:
        raise RuntimeError("shape_ftp did not return estimated_grating_period_px and OVERRIDE_MM_PER_PX is not set.")
    est = float(estimated_grating_period_px)
    if (not np.isfinite(est)) or est <= 1e-12:
        raise RuntimeError(f"Invalid estimated_grating_period_px={estimated_grating_period_px}.")
    return float(grating_pitch_mm) / est


def predict_force_from_volume(best_model: Dict[str, Any], volume_cm3: float) -> float:
    """force_sensor.predict_force_from_volume (Code/force_sensor.py:149-167) through the C ABI."""
    c = _curve(best_model, "force calibration JSON")
    out = ctypes.c_double()
    call(None, "vistaf_predict_force_from_volume", ctypes.byref(c), float(volume_cm3), ctypes.byref(out))
    return float(out.value)


def depth_map_to_volume_cm3(height_map_mm, roi_mask, mm_per_px: float, depth_eps_mm: float = 0.01, device="cuda:0"):
    """force_sensor.depth_map_to_volume_cm3 (Code/force_sensor.py:93-123) on the GPU.

    height_map_mm: [h,w] or [B,h,w] (numpy or torch); roi_mask: same shape bool/uint8 or None for
    isfinite(height).  Returns (volume_cm3, contact_area_mm2, max_depth_mm) floats, or a [B,3] array."""
    _lib.load()                                             # a missing library is reported before anything touches the device
    dev = torch.device(device)
    h_t = torch.as_tensor(np.asarray(height_map_mm, dtype=np.float32) if not torch.is_tensor(height_map_mm) else height_map_mm)
    single = h_t.dim() == 2
    if single:
        h_t = h_t[None]
    h_t = h_t.to(dev, torch.float32).contiguous()
    r_t = None
    if roi_mask is not None:
        r_t = torch.as_tensor(np.asarray(roi_mask) if not torch.is_tensor(roi_mask) else roi_mask)
        if r_t.dim() == 2:
            r_t = r_t[None]
        if r_t.shape != h_t.shape:
            raise ValueError("roi_mask shape does not match height_map_mm")
        r_t = r_t.to(dev).to(torch.uint8).contiguous()
    b, hh, ww = h_t.shape
    out = torch.empty((b, 3), dtype=torch.float64, device=dev)
    call(dev, "vistaf_depth_map_to_volume", h_t.data_ptr(), r_t.data_ptr() if r_t is not None else None, b, hh, ww, float(mm_per_px),
         float(depth_eps_mm), out.data_ptr(), stream(dev))
    res = out.cpu().numpy()
    if single:
        return float(res[0, 0]), float(res[0, 1]), float(res[0, 2])
    return res


# ---- input frame layouts (VISTAF_FMT_*, include/vistaf_ftp.h): device-free ---------------------------------------------------------------
_FORMAT_NAMES = {code: name for name, code in _lib.FORMATS.items()}
_F16_FORMATS = (_lib.FMT_GRAY_F16, _lib.FMT_BGR_F16)
_CHANNELS = {_lib.FMT_BGR_U8: 3, _lib.FMT_BGR_F16: 3, _lib.FMT_RGB_U8: 3, _lib.FMT_BGRA_U8: 4, _lib.FMT_RGBA_U8: 4}
_YUV422 = (_lib.FMT_YUYV_U8, _lib.FMT_UYVY_U8)
_ALIGN = {_lib.FMT_GRAY_F16: 2, _lib.FMT_BGR_F16: 2, _lib.FMT_BGRA_U8: 4, _lib.FMT_RGBA_U8: 4, _lib.FMT_YUYV_U8: 4, _lib.FMT_UYVY_U8: 4}


def _format_code(format) -> int:
    """a name of `_lib.FORMATS` or a VISTAF_FMT_* code -> the code; ValueError for anything else"""
    if isinstance(format, str):
        if format not in _lib.FORMATS:
            raise ValueError(f"unknown frame format {format!r}: one of {', '.join(_lib.FORMATS)}")
        return _lib.FORMATS[format]
    if isinstance(format, bool) or not isinstance(format, (int, np.integer)) or int(format) not in _FORMAT_NAMES:
        raise ValueError(f"unknown frame format {format!r}: a name of _lib.FORMATS or a code 0..{len(_FORMAT_NAMES) - 1}")
    return int(format)


def _frame_shapes(code: int, h: int, w: int):
    """the shapes one frame of h x w pixels may come in, the layout of the header's table first; ValueError where the format cannot hold the size"""
    name = _FORMAT_NAMES[code]
    if h < 1 or w < 1:
        raise ValueError(f"frame size {h} x {w} is below 1 x 1")
    if code in _CHANNELS:
        return [(h, w, _CHANNELS[code])]
    if code in _YUV422:
        if w % 2:
            raise ValueError(f"frame format {name} needs an even width, not {w}")
        return [(h, w // 2, 4), (h, 2 * w)]
    if code == _lib.FMT_NV12_U8:
        if h % 2 or w % 2:
            raise ValueError(f"frame format nv12 needs an even height and an even width, not {h} x {w}")
        return [(3 * h // 2, w), (3 * h * w // 2,)]
    if code >= _lib.FMT_BAYER_RGGB_U8 and (h < 2 or w < 2):
        raise ValueError(f"frame format {name} needs at least 2 x 2 pixels, not {h} x {w}")
    return [(h, w)]


def frame_layout(format, h: int, w: int):
    """One frame of h x w pixels in `format` (a name of `_lib.FORMATS` or a VISTAF_FMT_* code): (shape, dtype, nbytes).  A batch is
    [B, *shape]; its frames follow each other without padding.  yuyv / uyvy may also come as [h, 2w] and nv12 (shape [3h/2, w]: the Y plane,
    then the chroma rows) as [3hw/2].  ValueError for an unknown format and for a size the format cannot hold: yuyv / uyvy at odd w, nv12
    at odd h or w, a Bayer mosaic below 2 x 2.  Needs no device."""
    code = _format_code(format)
    shape = _frame_shapes(code, int(h), int(w))[0]
    dtype = torch.float16 if code in _F16_FORMATS else torch.uint8
    return shape, dtype, int(np.prod(shape)) * (2 if code in _F16_FORMATS else 1)


def _frame_size(code: int, shape) -> Tuple[int, int]:
    """(h, w) of a single frame of this shape (a leading batch dimension of 1 allowed): what a session reads off its reference frame"""
    shape = tuple(int(v) for v in shape)
    rank = 3 if code in _CHANNELS else 2
    if code in _YUV422 and len(shape) >= 3 and shape[-1] == 4:
        rank = 3
    if len(shape) == rank + 1 and shape[0] == 1:
        shape = shape[1:]
    bad = ValueError(f"a reference frame of shape {shape} is not one frame in format {_FORMAT_NAMES[code]}")
    if len(shape) != rank:
        raise bad
    if code in _YUV422:
        if rank == 2 and shape[1] % 2:
            raise bad
        return shape[0], shape[1] * 2 if rank == 3 else shape[1] // 2
    if code == _lib.FMT_NV12_U8:
        if shape[0] % 3:
            raise bad
        return shape[0] // 3 * 2, shape[1]
    return shape[0], shape[1]


class FtpSensor(Handle):
    """One FTP session: a reference frame, an ROI circle, constants and the two calibration curves.

    The reference frame is demodulated once on the GPU (Code/shape_ftp.py:1632-1639 does it on every
    call); `predict_batch` then runs Code/shape_ftp.py:1641-2037 + the force tail for B frames.
    """
    _destroy = "vistaf_ftp_destroy"

    def __init__(self, reference, roi_circle: Optional[Tuple[int, int, int]] = None, config: Optional[FtpConfig] = None,
                 height_model: Optional[Dict[str, Any]] = None, use_negated_height: bool = True,
                 force_model: Optional[Dict[str, Any]] = None, max_batch: int = 256, device="cuda:0",
                 frame_shape: Optional[Tuple[int, int]] = None, format=None):
        """reference: the session's reference frame, or None for a session that only runs `predict_pairs` (every sample then brings its
        own reference frame; `frame_shape` = (h, w) is needed instead).  format: the layout of `reference` (see `predict_batch`)."""
        self._readouts: Dict[str, Tuple[tuple, Any]] = {}          # the live read-outs: name -> (the parameters it was built with, the object)
        self._open(device)
        self.config = config or FtpConfig.as_shipped()
        if height_model is None or force_model is None:
            raise KeyError("height_model and force_model (the 'best_model' blocks of the calibration JSONs) are required")
        if reference is None:
            if frame_shape is None:
                raise ValueError("a session without a reference frame needs frame_shape=(h, w)")
            ref = None
            self.h, self.w = int(frame_shape[0]), int(frame_shape[1])
        elif format is not None:
            shape = reference.shape if hasattr(reference, "shape") else np.asarray(reference).shape
            self.h, self.w = _frame_size(_format_code(format), shape)
            ref, ref_format = self._frames_in(reference, format)
        else:
            ref = self._as_frames(reference)
            if ref.shape[0] != 1:
                raise ValueError("reference must be a single frame")
            self.h, self.w = int(ref.shape[1]), int(ref.shape[2])
            ref_format = self._format_of(ref)
        if roi_circle is None:
            roi_circle = (self.w // 2, self.h // 2, min(self.h, self.w) // 2 - 1)
        self.roi_circle = tuple(int(v) for v in roi_circle)
        self.max_batch = int(max_batch)
        self.height_model, self.force_model = height_model, force_model
        cc = self.config.to_c()
        hc, fc = _curve(height_model, "calibration"), _curve(force_model, "force calibration JSON")
        self._call("vistaf_ftp_create", ctypes.byref(cc), self.h, self.w, *self.roi_circle, self.max_batch, ctypes.byref(hc),
                   int(bool(use_negated_height)), ctypes.byref(fc), ctypes.byref(self._h))
        self.reference_info = None
        if ref is not None:
            self._call("vistaf_ftp_set_reference", self._h, ref.data_ptr(), ref_format, self._stream())
            info = (ctypes.c_double * _lib.NREFINFO)()
            self._call("vistaf_ftp_get_reference_info", self._h, info, on_device=False)
            self.reference_info = self._info_dict(info, 0)

    @staticmethod
    def _info_dict(info, o):
        return {
            "peak_refined": (info[o + 0], info[o + 1]), "k": (info[o + 2], info[o + 3]), "fft_shape": (int(info[o + 4]), int(info[o + 5])),
            "estimated_grating_period_px": info[o + 6], "mm_per_px": info[o + 7],
        }

    # -- helpers ---------------------------------------------------------------------------------
    def _as_frames(self, frames) -> torch.Tensor:
        t = frames if torch.is_tensor(frames) else torch.from_numpy(np.ascontiguousarray(frames))
        if t.dtype not in (torch.uint8, torch.float16):
            raise ValueError("frames must be uint8 or float16")
        if t.dim() == 2:
            t = t[None]
        elif t.dim() == 3 and t.shape[-1] == 3 and t.shape[0] != 3:
            t = t[None]                    # one HxWx3 frame
        if t.dim() not in (3, 4) or (t.dim() == 4 and t.shape[-1] != 3):
            raise ValueError("frames must be [h,w], [B,h,w], [h,w,3] or [B,h,w,3]")
        return t.to(self.device).contiguous()

    @staticmethod
    def _format_of(t: torch.Tensor) -> int:
        if t.dtype == torch.uint8:
            return _lib.FMT_BGR_U8 if t.dim() == 4 else _lib.FMT_GRAY_U8
        return _lib.FMT_BGR_F16 if t.dim() == 4 else _lib.FMT_GRAY_F16

    def _frames_in(self, frames, format) -> Tuple[torch.Tensor, int]:
        """(frames as a contiguous device tensor [B, ...], their VISTAF_FMT_* code).  format None: the format follows from dtype and rank
        (`_as_frames`, `_format_of`).  A name or a code: one frame or a batch in one of that format's shapes for the session's size
        (`frame_layout`), ValueError otherwise -- nothing is converted or reinterpreted on the way."""
        if format is None:
            t = self._as_frames(frames)
            if t.shape[1] != self.h or t.shape[2] != self.w:
                raise RuntimeError("Reference and deformed images have different sizes.")   # shape_ftp.py:1477-1478
            return t, self._format_of(t)
        code = _format_code(format)
        shapes = _frame_shapes(code, self.h, self.w)
        dtype = torch.float16 if code in _F16_FORMATS else torch.uint8
        t = frames if torch.is_tensor(frames) else torch.from_numpy(np.ascontiguousarray(frames))
        if t.dtype != dtype:
            raise ValueError(f"frames in format {_FORMAT_NAMES[code]} must be {dtype}, not {t.dtype}")
        if tuple(t.shape) in shapes:
            t = t[None]
        elif t.dim() < 2 or tuple(t.shape[1:]) not in shapes:
            raise ValueError(f"frames of shape {tuple(t.shape)} are not {self.h} x {self.w} frames in format {_FORMAT_NAMES[code]}: "
                             f"one frame is {' or '.join(str(list(v)) for v in shapes)}, a batch [B, ...] of that")
        t = t.to(self.device).contiguous()
        if t.data_ptr() % _ALIGN.get(code, 1):
            t = t.clone()                  # a view that starts below the alignment the format's kernel loads with
        return t, code

    def close(self):
        for name in list(getattr(self, "_readouts", {})):
            self._readouts.pop(name)[1].close()
        super().close()

    # -- the session's read-outs ------------------------------------------------------------------
    def _matching(self, name: str, key: tuple, reset: Optional[bool] = None, differ: str = ""):
        """The live read-out `name` if it was built with the parameters `key`, else None.  One built with other parameters is closed:
        always when reset is None (the read-out is rebuilt silently), only with reset=True otherwise, ValueError(differ) without."""
        live = self._readouts.get(name)
        if live is None or live[0] == key:
            return live and live[1]
        if reset is False:
            raise ValueError(differ)
        self._readouts.pop(name)[1].close()
        return None

    def _keep(self, name: str, key: tuple, readout):
        self._readouts[name] = (key, readout)
        return readout

    def _table_and(self, name: str, key: tuple, make):
        """The contacts dict of the last predict for key[0] rows, with the index plane, and the session's read-out `name` built with the
        parameters `key`: the live one, else make() -- called after the table is read, so a session without a predict builds nothing."""
        live = self._matching(name, key)
        out = self.contacts(key[0], index_plane=True)
        return out, live if live is not None else self._keep(name, key, make())

    def _live(self, name: str):
        live = getattr(self, "_readouts", {}).get(name)
        return live and live[1]

    _tracker = property(lambda self: self._live("tracker"))
    _shapes = property(lambda self: self._live("shapes"))
    _taxels = property(lambda self: self._live("taxels"))
    _thermal = property(lambda self: self._live("thermal"))
    _temporal = property(lambda self: self._live("temporal"))
    _cloud = property(lambda self: self._live("cloud"))
    _motion = property(lambda self: self._live("motion"))
    _pressure = property(lambda self: self._live("pressure"))
    _outlines = property(lambda self: self._live("outlines"))
    _textures = property(lambda self: self._live("textures"))
    _matches = property(lambda self: self._live("matches"))
    _centrelines = property(lambda self: self._live("centrelines"))
    _lobes = property(lambda self: self._live("lobes"))

    def _last(self, who: str, what: str = "predict_batch / predict_pairs") -> Dict[str, torch.Tensor]:
        last = getattr(self, "_last_out", None)
        if last is None:
            raise RuntimeError(f"{who}() needs a previous {what}")
        return last

    def _scalar(self, name: str) -> torch.Tensor:
        """the column `name` of the last predict's scalars"""
        return self._last_out["scalars"][:, SCALAR_NAMES.index(name)]

    def _new_out(self, b: int) -> Dict[str, torch.Tensor]:
        return {
            "height_map_mm": torch.empty((b, self.h, self.w), dtype=torch.float32, device=self.device),
            "output_reliable": torch.empty((b, self.h, self.w), dtype=torch.uint8, device=self.device),
            "scalars": torch.empty((b, _lib.NSCALARS), dtype=torch.float64, device=self.device),
            "status": torch.empty((b,), dtype=torch.int32, device=self.device),
        }

    # -- batched device API ------------------------------------------------------------------------
    def predict_batch(self, frames, out: Optional[Dict[str, torch.Tensor]] = None, format=None) -> Dict[str, torch.Tensor]:
        """frames: [B,h,w] or [B,h,w,3], uint8 or float16 (device or host), or, with format= a name of `_lib.FORMATS` ("rgb", "bgra",
        "rgba", "yuyv", "uyvy", "nv12", "bayer_rggb", ...) or a VISTAF_FMT_* code, frames in that layout (`frame_layout`; ValueError when
        they are not).  Returns device tensors:
        height_map_mm [B,h,w] f32 (NaN outside ROI), output_reliable [B,h,w] u8, scalars [B,16] f64, status [B] i32."""
        t, code = self._frames_in(frames, format)
        b = int(t.shape[0])
        if b > self.max_batch:
            raise RuntimeError(f"batch {b} exceeds max_batch {self.max_batch}")
        if out is None:
            out = self._new_out(b)
        self._call("vistaf_ftp_predict_batch", self._h, t.data_ptr(), code, b, out["height_map_mm"].data_ptr(),
                   out["output_reliable"].data_ptr(), out["scalars"].data_ptr(), out["status"].data_ptr(), self._stream())
        self._last_out = out
        return out

    def predict_pairs(self, references, frames, out: Optional[Dict[str, torch.Tensor]] = None, format=None) -> Dict[str, torch.Tensor]:
        """Uncached pairs: sample b = (references[b], frames[b]); every sample's reference frame is demodulated with its own carrier
        search, as Code/height_to_force.py:384 does by calling shape_ftp.main once per image.  Same outputs as predict_batch; status 3
        marks a sample whose reference spectrum holds no usable carrier.  format: the layout of both frame sets, as in `predict_batch`."""
        (r, rcode), (t, code) = self._frames_in(references, format), self._frames_in(frames, format)
        if r.shape != t.shape or rcode != code:
            if format is None:
                raise RuntimeError("Reference and deformed images have different sizes.")   # shape_ftp.py:1477-1478
            raise ValueError(f"{r.shape[0]} reference frames for {t.shape[0]} deformed frames")
        b = int(t.shape[0])
        if b > self.max_batch:
            raise RuntimeError(f"batch {b} exceeds max_batch {self.max_batch}")
        if out is None:
            out = self._new_out(b)
        self._call("vistaf_ftp_predict_pairs", self._h, r.data_ptr(), t.data_ptr(), code, b, out["height_map_mm"].data_ptr(),
                   out["output_reliable"].data_ptr(), out["scalars"].data_ptr(), out["status"].data_ptr(), self._stream())
        self._last_out = out
        return out

    def pair_info(self, batch: int):
        """reference_info of every sample of the last predict_pairs"""
        info = (ctypes.c_double * (_lib.NREFINFO * batch))()
        self._call("vistaf_ftp_get_pair_info", self._h, batch, info, self._stream())
        return [self._info_dict(info, b * _lib.NREFINFO) for b in range(batch)]

    def contacts(self, max_contacts: int = 8, index_plane: bool = False) -> Dict[str, torch.Tensor]:
        """Per-contact table of the last predict_batch / predict_pairs (vistaf_ftp_contacts; an extension, the reference has no
        counterpart).  A contact is one 8-connected component of the `contact_kept_by_depth` mask; per frame they are ordered by maximum
        depth, descending.  Returns device tensors: contacts [B,K,16] f64 (fields CONTACT_NAMES, unused rows NaN), count [B] i32 (all
        contacts of the frame, also when more than K) and, with index_plane, contact_index [B,h,w] i8 (row of the pixel's contact, else -1).
        `force_N` of a row is the force curve at that contact's own volume; the curve is not linear, the rows do not add up to the frame's."""
        last = self._last("contacts")
        b, k = int(last["status"].shape[0]), int(max_contacts)
        if not 1 <= k <= _lib.MAX_CONTACTS:
            raise ValueError(f"max_contacts must be 1..{_lib.MAX_CONTACTS}")
        out = {
            "contacts": torch.empty((b, k, _lib.NCONTACT), dtype=torch.float64, device=self.device),
            "count": torch.empty((b,), dtype=torch.int32, device=self.device),
        }
        if index_plane:
            out["contact_index"] = torch.empty((b, self.h, self.w), dtype=torch.int8, device=self.device)
        self._call("vistaf_ftp_contacts", self._h, b, k, out["contacts"].data_ptr(), out["count"].data_ptr(),
                   out["contact_index"].data_ptr() if index_plane else None, self._stream())
        return out

    def track(self, max_contacts: int = 8, gate_px: float = 0.0, reset: bool = False) -> Dict[str, torch.Tensor]:
        """Per-contact table of the last predict plus its link to the frames before it (tracks.ContactTracker; an extension, the reference
        has no counterpart).  Calls `contacts(max_contacts, index_plane=True)` and hands the result to the session's tracker, created on
        first use: the frames of this predict follow the frames of the predict of the previous `track` call.  Returns the contacts dict
        plus tracks [B,K,16] f64 (fields TRACK_NAMES: persistent id, age, parent row, events, overlap, motion) and fate [B,K] i32.
        reset=True forgets the frames seen so far and restarts ids at 0; max_contacts and gate_px can only change together with it."""
        from .tracks import ContactTracker
        k, gate = int(max_contacts), float(gate_px)
        tr = self._matching("tracker", (k, gate), bool(reset), "max_contacts / gate_px differ from the running tracker's: pass reset=True to start over with them")
        out = self.contacts(k, index_plane=True)
        if tr is None:
            tr = self._keep("tracker", (k, gate), ContactTracker(self.h, self.w, self.max_batch, k, gate, device=self.device))
        elif reset:
            tr.reset()
        out.update(tr.update(out["contact_index"], out["contacts"], out["count"]))
        return out

    def shapes(self, max_contacts: int = 8, fit_min_fraction: float = 0.5) -> Dict[str, torch.Tensor]:
        """Per-contact table of the last predict plus the shape of every contact (shapes.ContactShapes; an extension, the reference has no
        counterpart).  Calls `contacts(max_contacts, index_plane=True)` and hands it, the predict's height map, the frames' mm_per_px (the
        `scalars` column) and the session's depth_eps_mm to the session's shape read-out, created on first use and rebuilt when
        max_contacts or fit_min_fraction change.  Returns the contacts dict plus shapes [B,K,24] f64 (fields SHAPE_NAMES: footprint
        ellipse, boundary pixels, apex, curvatures and radii of the fitted cap, residual)."""
        from .shapes import ContactShapes
        k, frac = int(max_contacts), float(fit_min_fraction)
        out, sh = self._table_and("shapes", (k, frac), lambda: ContactShapes(self.h, self.w, self.max_batch, k, frac, device=self.device))
        out["shapes"] = sh.measure(self._last_out["height_map_mm"], out["contact_index"], out["contacts"], out["count"], self._scalar("mm_per_px"),
                                   self.config.depth_eps_mm)
        return out

    def outlines(self, max_contacts: int = 8, max_vertices: Optional[int] = None) -> Dict[str, torch.Tensor]:
        """Per-contact table of the last predict plus the outline of every contact (outline.contact_outlines; an extension, the reference has
        no counterpart).  Calls `contacts(max_contacts, index_plane=True)` and hands it and the frames' mm_per_px (the `scalars` column) to
        the outline read-out; its workspace is the session's, made on first use and again when max_contacts changes.  Returns the contacts
        dict plus outlines [B,K,24] f64 (fields OUTLINE_NAMES: loops, holes, perimeter, hull, Feret diameters, caliper box), vertices
        [B,V,2] i32 and offsets [B,K+1] i32, the corner polylines of the principal loops (`outline.trim` cuts them).  max_vertices: V per
        frame, by default 4 * (h + w) (`outline.default_max_vertices`); rows that do not fit show corners_written < corners; 0: no polylines."""
        from .outline import OutlineWorkspace, contact_outlines
        k = int(max_contacts)
        out, ws = self._table_and("outlines", (k,), lambda: OutlineWorkspace(self.h, self.w, self.max_batch, k, self.device))
        out.update(contact_outlines(out["contact_index"], out["contacts"], out["count"], self._scalar("mm_per_px"), max_vertices, ws))
        return out

    def textures(self, max_contacts: int = 8, **params) -> Dict[str, torch.Tensor]:
        """Per-contact table of the last predict plus the surface texture of every contact (texture.contact_textures; an extension, the
        reference has no counterpart).  Calls `contacts(max_contacts, index_plane=True)` and hands it, the predict's height map, the frames'
        mm_per_px (the `scalars` column) and the session's depth_eps_mm to the texture read-out; its workspace is the session's, made on
        first use and again when max_contacts or max_lag change.  params: the keyword arguments of `contact_textures` (eval_min_fraction,
        form_degree, max_lag, acf_threshold, peak_min).  Returns the contacts dict plus textures [B,K,40] f64 (fields TEXTURE_NAMES:
        form, roughness, gradient direction and coherence, lobe, pitch), residual [B,h,w] f32 and acf [B,K,2L+1,2L+1] f64."""
        from .texture import TextureWorkspace, contact_textures
        unknown = set(params) - {"eval_min_fraction", "form_degree", "max_lag", "acf_threshold", "peak_min"}
        if unknown:
            raise TypeError(f"textures() got unexpected keyword arguments {sorted(unknown)}")
        k, lag = int(max_contacts), int(params.get("max_lag", 8))
        out, ws = self._table_and("textures", (k, lag), lambda: TextureWorkspace(self.h, self.w, self.max_batch, k, lag, self.device))
        out.update(contact_textures(self._last_out["height_map_mm"], out["contact_index"], out["contacts"], out["count"], self._scalar("mm_per_px"),
                                    self.config.depth_eps_mm, ws, **params))
        return out

    def matches(self, bank, max_contacts: int = 8, **params) -> Dict[str, torch.Tensor]:
        """Per-contact table of the last predict plus the known indenter every contact matches (match.contact_matches; an extension, the
        reference has no counterpart).  Calls `contacts(max_contacts, index_plane=True)` and hands it, the predict's height map, the frames'
        mm_per_px (the `scalars` column) and the session's depth_eps_mm to the match read-out with `bank` (a match.TemplateBank); its
        workspace is the session's, made on first use and again when max_contacts, max_shift or the bank's sizes change.  params: the keyword
        arguments of `contact_matches` (max_shift, min_pixels, accept_score, accept_margin).  Returns the contacts dict plus matches [B,K,24]
        f64 (fields MATCH_NAMES: status, label, template, rotation, position, scores, fit), scores [B,K,T] f64 and patches [B,K,S,S] f32."""
        from .match import MatchWorkspace, TemplateBank, contact_matches
        unknown = set(params) - {"max_shift", "min_pixels", "accept_score", "accept_margin"}
        if unknown:
            raise TypeError(f"matches() got unexpected keyword arguments {sorted(unknown)}")
        if not isinstance(bank, TemplateBank):
            raise TypeError("bank must be a match.TemplateBank")
        k, m = int(max_contacts), int(params.get("max_shift", 3))
        out, ws = self._table_and("matches", (k, bank.P, m, bank.M), lambda: MatchWorkspace(self.h, self.w, self.max_batch, k, bank.P, m, bank.M, self.device))
        out.update(contact_matches(self._last_out["height_map_mm"], out["contact_index"], out["contacts"], out["count"], self._scalar("mm_per_px"),
                                   self.config.depth_eps_mm, bank, ws, **params))
        return out

    def centrelines(self, max_contacts: int = 8, max_stations: Optional[int] = None, **params) -> Dict[str, torch.Tensor]:
        """Per-contact table of the last predict plus the centreline of every contact (centreline.contact_centrelines; an extension, the
        reference has no counterpart).  Calls `contacts(max_contacts, index_plane=True)` and hands it, the predict's height map (the depth
        plane of the DEPTH_* fields) and the frames' mm_per_px (the `scalars` column) to the centreline read-out; its workspace is the
        session's, made on first use and again when max_contacts changes.  params: tangent_span (default 8), skeleton (default True).
        Returns the contacts dict plus centrelines [B,K,40] f64 (fields CENTRELINE_NAMES: skeleton counts, ends, lengths, bend, widths,
        tangents, border flags, depth along the path), stations [B,V,2] i32, station_d2 [B,V] i32 and offsets [B,K+1] i32, the axis paths
        and their squared half-widths (`centreline.trim` cuts them), and skeleton [B,h,w] i8.  max_stations: V per frame, by default
        2 * (h + w) (`centreline.default_max_stations`); rows that do not fit show stations_written < stations; 0: no polylines."""
        from .centreline import CentrelineWorkspace, contact_centrelines
        unknown = set(params) - {"tangent_span", "skeleton"}
        if unknown:
            raise TypeError(f"centrelines() got unexpected keyword arguments {sorted(unknown)}")
        k = int(max_contacts)
        out, ws = self._table_and("centrelines", (k,), lambda: CentrelineWorkspace(self.h, self.w, self.max_batch, k, self.device))
        out.update(contact_centrelines(out["contact_index"], out["contacts"], out["count"], self._scalar("mm_per_px"), self._last_out["height_map_mm"],
                                       max_stations=max_stations, workspace=ws, **params))
        return out

    def lobes(self, max_contacts: int = 8, max_lobes: int = 4, min_prominence_mm: Optional[float] = None,
              min_prominence_frac: Optional[float] = None, split: bool = True) -> Dict[str, torch.Tensor]:
        """Per-contact table of the last predict plus the lobes every contact splits into at the saddles of its depth relief
        (lobes.contact_lobes; an extension, the reference has no counterpart): two fingertips whose footprints joined are one row of the
        contacts table and two lobes here.  Calls `contacts(max_contacts, index_plane=True)` and hands it, the predict's height map, the
        frames' mm_per_px (the `scalars` column) and the session's depth_eps_mm to the lobe read-out; its workspace is the session's, made
        on first use and again when max_contacts changes.  min_prominence_mm / min_prominence_frac: None takes the defaults of `lobes`
        (0.02 mm and 0.10 of the contact's greatest depth: a judgement about noise nobody has measured on this sensor).  Returns the
        contacts dict plus lobes [B,K,max_lobes,16] f64 (fields LOBE_NAMES), lobe_rows [B,K,12] f64 (fields LOBE_ROW_NAMES), lobe_index
        [B,h,w] i8 and, with split, split_contacts [B,K,16] f64, split_count [B] i32, split_index [B,h,w] i8 -- the lobes as a contacts
        table the tracker and the other read-outs take unchanged; its force_N is each lobe's share of its parent's force -- and
        split_parent [B,K,2] i32."""
        from .lobes import DEFAULT_MIN_PROMINENCE_FRAC, DEFAULT_MIN_PROMINENCE_MM, LobesWorkspace, contact_lobes
        k = int(max_contacts)
        out, ws = self._table_and("lobes", (k,), lambda: LobesWorkspace(self.h, self.w, self.max_batch, k, self.device))
        out.update(contact_lobes(out["contact_index"], out["contacts"], out["count"], self._scalar("mm_per_px"), self._last_out["height_map_mm"],
                                 max_lobes=max_lobes, min_prominence_mm=DEFAULT_MIN_PROMINENCE_MM if min_prominence_mm is None else min_prominence_mm,
                                 min_prominence_frac=DEFAULT_MIN_PROMINENCE_FRAC if min_prominence_frac is None else min_prominence_frac,
                                 depth_eps_mm=self.config.depth_eps_mm, split=split, workspace=ws))
        return out

    def taxels(self, layout) -> Dict[str, torch.Tensor]:
        """Taxel read-out of the last predict (taxels.TaxelReadout; an extension, the reference has no counterpart): the height map reduced to
        the fixed cells of `layout` (taxels.grid_layout, polar_layout, from_map) and to the frame's wrench.  Hands the predict's height map,
        the frames' mm_per_px and force_N (the `scalars` columns), their status and the session's depth_eps_mm to the session's read-out,
        created on first use and rebuilt when another layout object is given.  Returns device tensors: taxels [B,T,12] f64 (fields
        TAXEL_NAMES) and frame [B,8] f64 (fields TAXEL_FRAME_NAMES); a frame whose status is not 0 has NaN rows."""
        from .taxels import TaxelReadout
        last = self._last("taxels")
        if layout.shape != (self.h, self.w):
            raise ValueError(f"the layout is {layout.shape[0]} x {layout.shape[1]}, the session's frames are {self.h} x {self.w}")
        tx = self._matching("taxels", (layout,))                  # the layout by identity: it defines no equality
        if tx is None:
            tx = self._keep("taxels", (layout,), TaxelReadout(layout, self.max_batch, device=self.device))
        return tx.measure(last["height_map_mm"], self._scalar("mm_per_px"), self.config.depth_eps_mm, force_N=self._scalar("force_N"),
                          status=last["status"])

    def thermal(self, temperature_crop, max_contacts: int = 8, surround_margin_px: int = 8) -> Dict[str, torch.Tensor]:
        """Per-contact table of the last predict plus the temperature of every contact (thermal.ThermalReadout; an extension, the reference has
        no counterpart).  `temperature_crop` [B,h,w] f32 is the caller's: a temperature map registered into the aligned crop by
        `ThermalReadout.register`.  Calls `contacts(max_contacts, index_plane=True)` and hands it, the predict's height map and status and the
        session's depth_eps_mm to the session's read-out, created on first use and rebuilt when max_contacts or surround_margin_px change.
        Returns the contacts dict plus thermal [B,K,16] f64 (fields THERMAL_NAMES) and thermal_frame [B,8] f64 (fields THERMAL_FRAME_NAMES)."""
        from .thermal import ThermalReadout
        k, margin = int(max_contacts), int(surround_margin_px)
        # measure needs the crop's size only; the photograph's is register's business
        out, th = self._table_and("thermal", (k, margin), lambda: ThermalReadout(self.h, self.w, max(self.h, 2), max(self.w, 2), (0, 0), False, self.max_batch,
                                                                                 k, margin, device=self.device))
        last = self._last_out
        r = th.measure(temperature_crop, last["height_map_mm"], out["contact_index"], out["contacts"], out["count"], self.config.depth_eps_mm,
                       status=last["status"])
        out["thermal"], out["thermal_frame"] = r["thermal"], r["frame"]
        return out

    def temporal(self, alpha: float = 0.5, on_mm: float = 0.05, off_mm: float = 0.02, frame_period_s: float = 1.0 / 30.0, reset: bool = False,
                 planes: bool = False) -> Dict[str, torch.Tensor]:
        """Temporal read-out of the last predict (temporal.TemporalReadout; an extension, the reference has no counterpart): every pixel's
        filtered depth, rate, touch bit, dwell and peak hold, carried from call to call.  Hands the predict's height map, the frames'
        mm_per_px (the `scalars` column) and their status to the session's read-out, created on first use: the frames of this predict follow
        the frames of the predict of the previous `temporal` call.  Returns device tensors: frames [B,16] f64 (fields TEMPORAL_NAMES) and,
        with planes=True, filtered [B,h,w] f32 and touch [B,h,w] u8.  reset=True forgets the stream; alpha, on_mm, off_mm and
        frame_period_s can only change together with it."""
        from .temporal import TemporalReadout
        last = self._last("temporal")
        prm = (float(alpha), float(on_mm), float(off_mm), float(frame_period_s))
        tp = self._matching("temporal", prm, bool(reset),
                            "alpha / on_mm / off_mm / frame_period_s differ from the running read-out's: pass reset=True to start over with them")
        if tp is None:
            tp = self._keep("temporal", prm, TemporalReadout(self.h, self.w, self.max_batch, *prm, device=self.device))
        elif reset:
            tp.reset()
        return tp.update(last["height_map_mm"], self._scalar("mm_per_px"), status=last["status"], planes=planes)

    def cloud(self, max_points: Optional[int] = None, stride: int = 1, labels: bool = False, max_contacts: int = 8) -> Dict[str, torch.Tensor]:
        """Point-cloud read-out of the last predict (cloud.CloudReadout; an extension, the reference has no counterpart): the surface pixels
        (depth > the session's depth_eps_mm) of every frame, every stride-th column and row, as points in millimetres about the crop centre
        with a unit normal, mean and Gaussian curvature each.  Hands the predict's height map, the frames' mm_per_px (the `scalars` column)
        and their status to the session's read-out, created on first use and rebuilt when max_points or stride change; labels=True also
        hands over the index plane of `contacts(max_contacts, index_plane=True)`.  Returns device tensors: points [max_points,8] f32 (fields
        CLOUD_POINT_NAMES), pixel [max_points] i32, label [max_points] i8 (with labels=True), offsets [B+1] i64, frame [B,12] f64 (fields
        CLOUD_FRAME_NAMES); `CloudReadout.trim` cuts the written part.  The default max_points is the lattice pixels of one frame or one
        eighth of those of max_batch frames, whichever is larger -- a sizing choice (a contact covers a small part of the crop), not a
        measurement.  More points than max_points is reported (offsets beyond max_points, points_written below points, `trim`'s overflow),
        not raised."""
        from .cloud import CloudReadout
        last = self._last("cloud")
        stride = int(stride)
        if max_points is None:
            lattice = ((self.h + stride - 1) // stride) * ((self.w + stride - 1) // stride) if stride >= 1 else 1
            max_points = max(lattice, (lattice * self.max_batch + 7) // 8)
        key = (int(max_points), stride)
        cl = self._matching("cloud", key) or self._keep("cloud", key, CloudReadout(self.h, self.w, self.max_batch, *key, device=self.device))
        index = self.contacts(int(max_contacts), index_plane=True)["contact_index"] if labels else None
        return cl.measure(last["height_map_mm"], self._scalar("mm_per_px"), self.config.depth_eps_mm, status=last["status"], contact_index=index)

    def motion(self, max_contacts: int = 8, gate_px: float = 0.0, reset: bool = False, iterations: int = 8, tol_px: float = 1e-3,
               min_pixels: int = 16, init_from_centroid: bool = True) -> Dict[str, torch.Tensor]:
        """Per-contact table of the last predict, its link to the frames before it and the motion of every linked contact against the skin
        (motion.ContactMotion; an extension, the reference has no counterpart).  Calls `track(max_contacts, gate_px, reset)` -- the tracker
        it needs -- and hands its result, the predict's height map, the frames' mm_per_px (the `scalars` column) and the session's
        depth_eps_mm to the session's motion read-out, created on first use: the frames of this predict follow the frames of the predict
        of the previous `motion` call, so `track` must not be called in between.  Returns the dict of `track` plus motion [B,K,24] f64
        (fields MOTION_NAMES: slide tx / ty, twist theta, depth change beta, residuals, standard errors) and motion_frame [B,8] f64 (fields
        MOTION_FRAME_NAMES).  reset=True forgets the frames seen so far; the other arguments can only change together with it."""
        from .motion import ContactMotion
        k = int(max_contacts)
        par = (k, int(iterations), float(tol_px), int(min_pixels), bool(init_from_centroid))
        mo = self._matching("motion", par, bool(reset), "the arguments differ from the running motion read-out's: pass reset=True to start over with them")
        out = self.track(k, gate_px, reset)
        if mo is None:
            mo = self._keep("motion", par, ContactMotion(self.h, self.w, self.max_batch, *par, device=self.device))
        elif reset:
            mo.reset()
        out.update(mo.update(self._last_out["height_map_mm"], out["contact_index"], out["contacts"], out["count"], out["tracks"],
                             self._scalar("mm_per_px"), self.config.depth_eps_mm))
        return out

    def pressure(self, max_contacts: int = 8, pad_px: int = 32, E_mpa: float = 1.0, nu: float = 0.45, thickness_mm: float = math.inf,
                 reset: bool = False) -> Dict[str, torch.Tensor]:
        """Per-contact table of the last predict plus the contact pressure map of an elastic skin under its height map
        (pressure.PressureReadout; an extension, the reference has no counterpart).  E_mpa, nu and thickness_mm (math.inf: a half-space)
        describe the skin and are the caller's: the package holds no material data, and the defaults are placeholders, not measurements.
        Calls `contacts(max_contacts, index_plane=True)` and hands it, the predict's height map, the frames' mm_per_px and force_N (the
        `scalars` columns), their status and the session's depth_eps_mm to the session's read-out, created on first use.  Returns the
        contacts dict plus pressure_kpa [B,h,w] f32, pressure [B,K,16] f64 (fields PRESSURE_NAMES) and pressure_frame [B,12] f64 (fields
        PRESSURE_FRAME_NAMES).  The other arguments can only change together with reset=True, which rebuilds the read-out with them."""
        from .pressure import PressureReadout
        k = int(max_contacts)
        par = (k, int(pad_px), float(E_mpa), float(nu), float(thickness_mm))
        pr = self._matching("pressure", par, bool(reset), "the arguments differ from the running pressure read-out's: pass reset=True to start over with them")
        out = self.contacts(k, index_plane=True)
        if pr is None:
            pr = self._keep("pressure", par, PressureReadout(self.h, self.w, self.max_batch, *par, device=self.device))
        last = self._last_out
        r = pr.measure(last["height_map_mm"], self._scalar("mm_per_px"), self.config.depth_eps_mm, contact_index=out["contact_index"],
                       contacts=out["contacts"], count=out["count"], force_N=self._scalar("force_N"), status=last["status"])
        out["pressure_kpa"], out["pressure"], out["pressure_frame"] = r["pressure_kpa"], r["rows"], r["frame"]
        return out

    def intermediate(self, name: str, batch: int, dtype=torch.float32) -> torch.Tensor:
        """Copy of a named intermediate plane of the last predict_batch (parity tests)."""
        per = ctypes.c_size_t()
        self._call("vistaf_ftp_get_intermediate", self._h, name.encode(), None, batch, ctypes.byref(per), None, on_device=False)
        nbytes = per.value * (batch if name not in ("roi", "cref", "amp_ref") else 1)
        buf = torch.empty((nbytes,), dtype=torch.uint8, device=self.device)
        self._call("vistaf_ftp_get_intermediate", self._h, name.encode(), buf.data_ptr(), batch, ctypes.byref(per), self._stream())
        torch.cuda.synchronize(self.device)
        return buf.view(dtype)

    def _test_set(self, name: str, value: int):
        """Test hook (csrc/test_hooks.h, not part of the boundary): select a fallback / opt-in kernel tier of a stage
        ("inpaint_tier", "big_flood_handback", "chamfer_twopass", "telea_two_tier", "telea_mw", "unwrap_fast", "big_chain", "big_queue_lds",
        "big_gq_cap", "big_fallback", "fused_chains", "fused_backend", "fused_masks", "select_resident", "dft_staged", "gauss_strip", "fit_window") or keep debug planes ("keep_planes")."""
        self._call("vistaf_ftp_test_set", self._h, name.encode(), int(value), on_device=False)

    def masks(self, index: int = 0) -> Dict[str, np.ndarray]:
        """The seven boolean crop masks of frame `index` of the last predict_batch, under the names the reference stores
        them with in height_map_bundle.npz (Code/shape_ftp.py:1898-1906)."""
        last = self._last("masks", "predict_batch")
        batch = int(last["status"].shape[0])

        def plane(name):
            return self.intermediate(name, batch, torch.uint8).view(batch, self.h, self.w)[index].cpu().numpy().astype(bool)
        roi = self.intermediate("roi", 1, torch.uint8).view(self.h, self.w).cpu().numpy().astype(bool)
        cx, cy, r = self.roi_circle
        yy, xx = np.ogrid[:self.h, :self.w]
        circ = ((xx - cx) ** 2 + (yy - cy) ** 2) <= r * r                                   # create_circular_mask (:437-440)
        reliable = plane("reliable")
        # hole candidates exist only without the reliable-region smoothing (Code/shape_ftp.py:1770-1801); otherwise upstream stores zeros too
        holes = plane("hole_cand") if not (self.config.reliable_smooth_sigma_px > 0) else np.zeros((self.h, self.w), dtype=bool)
        return {
            "roi_eroded": roi, "reliable": reliable, "output_reliable": last["output_reliable"][index].cpu().numpy().astype(bool), "circ_mask": circ,
            "contact_kept_by_depth": plane("kept"), "hole_candidates": holes,
            "contact_dilated": plane("contact_d"),
        }

    def enable_stage_timing(self, enable: bool = True):
        self._call("vistaf_ftp_enable_stage_timing", self._h, int(enable), on_device=False)

    def stage_times_ms(self) -> Dict[str, float]:
        n = self._lib.vistaf_ftp_stage_count()
        arr = (ctypes.c_float * n)()
        self._call("vistaf_ftp_get_stage_times", self._h, arr, n, on_device=False)
        return {self._lib.vistaf_ftp_stage_name(i).decode(): float(arr[i]) for i in range(n)}

    # -- single-frame API in the reference's vocabulary ---------------------------------------------
    def predict(self, image, contacts: Optional[int] = None, shapes: bool = False, taxels=None, thermal=None,
                temporal: Optional[Dict[str, Any]] = None, cloud: Optional[Dict[str, Any]] = None,
                motion: Optional[Dict[str, Any]] = None, pressure: Optional[Dict[str, Any]] = None, format=None,
                outlines: bool = False, textures: Optional[Dict[str, Any]] = None,
                matches: Optional[Dict[str, Any]] = None, centrelines=False, lobes=False) -> Optional[Dict[str, Any]]:
        """One deformed frame -> the dict shape_ftp.main(..., return_results=True) returns
        (Code/shape_ftp.py:2029-2037) plus the force tail of multimodal_sensor.py:388-419.
        Returns None when the reliable mask is empty, as upstream does (shape_ftp.py:1677-1679).
        format: the layout of `image`, as in `predict_batch`.
        contacts=K adds a "contacts" key: the frame's (at most K) contacts as dicts of CONTACT_NAMES plus `centroid_xy`, `argmax_xy` and
        `bbox` in crop coordinates, and "contact_count"; without it the dict has exactly the reference's keys plus the scalars.
        shapes=True (with contacts=K) adds a "shapes" key: one dict of SHAPE_NAMES per entry of "contacts" (`FtpSensor.shapes`).
        taxels=layout adds "taxels", the ndarray [T,12] of `FtpSensor.taxels` (fields TAXEL_NAMES), and "taxel_frame", a dict of
        TAXEL_FRAME_NAMES (active_taxels and peak_taxel as ints, peak_taxel -1 without contact).
        thermal=temperature_crop (with contacts=K; [h,w] f32 from `ThermalReadout.register`) adds "thermal", one dict of THERMAL_NAMES per
        entry of "contacts", and "thermal_frame", a dict of THERMAL_FRAME_NAMES (`FtpSensor.thermal`).
        temporal=dict(...) (the keyword arguments of `FtpSensor.temporal` but `planes`) adds "temporal_frame", a dict of TEMPORAL_NAMES:
        this frame follows the frame of the previous predict that asked for it.  A frame for which None is returned or an error raised
        does not reach the read-out.
        cloud=dict(...) (the keyword arguments of `FtpSensor.cloud`, possibly none) adds "cloud", the ndarray [N,8] of the frame's written
        points (fields CLOUD_POINT_NAMES), "cloud_pixel", their pixel indices [N], "cloud_label" [N] with labels=True, and "cloud_frame", a
        dict of CLOUD_FRAME_NAMES.
        motion=dict(...) (with contacts=K; the keyword arguments of `FtpSensor.motion` but `max_contacts`, possibly none) adds "tracks", one
        dict of TRACK_NAMES per entry of "contacts", "motion", one dict of MOTION_NAMES per entry, and "motion_frame", a dict of
        MOTION_FRAME_NAMES: this frame follows the frame of the previous predict that asked for it.
        pressure=dict(...) (the keyword arguments of `FtpSensor.pressure` but `max_contacts`: E_mpa, nu, thickness_mm, pad_px) adds
        "pressure_kpa", the ndarray [h,w] f32 of the contact pressure, "pressure_frame", a dict of PRESSURE_FRAME_NAMES, and, with contacts=K,
        "pressure", one dict of PRESSURE_NAMES per entry of "contacts".
        outlines=True (with contacts=K) adds "outlines", one dict of OUTLINE_NAMES per entry of "contacts" (`FtpSensor.outlines`), and
        "outline_polylines", per entry the [n,2] list of its principal loop's corners (None for a row that did not fit the capacity).
        textures=dict(...) (with contacts=K; the keyword arguments of `FtpSensor.textures` but `max_contacts`, possibly none) adds "textures",
        one dict of TEXTURE_NAMES per entry of "contacts".
        matches=dict(bank=..., ...) (with contacts=K; `bank` a match.TemplateBank and the keyword arguments of `FtpSensor.matches` but
        `max_contacts`) adds "matches", one dict of MATCH_NAMES per entry of "contacts".
        centrelines=True or dict(...) (with contacts=K; the keyword arguments of `FtpSensor.centrelines` but `max_contacts` and `skeleton`)
        adds "centrelines", one dict of CENTRELINE_NAMES per entry of "contacts", "centreline_stations", per entry the [n,2] list of its axis
        path from A to B (None for a row that did not fit the capacity), and "centreline_d2", per entry the squared half-widths along it.
        lobes=True or dict(...) (with contacts=K; the keyword arguments of `FtpSensor.lobes` but `max_contacts` and `split`) adds "lobes",
        per entry of "contacts" the list of its written lobes as dicts of LOBE_NAMES, "lobe_rows", one dict of LOBE_ROW_NAMES per entry, and
        "split_contacts", the lobes of the frame as a contacts list of their own (dicts of CONTACT_NAMES plus `parent`, the (row, lobe) each
        came from; `force_N` is the lobe's share of its parent's force)."""
        want_lobes = lobes is not None and lobes is not False
        if want_lobes and contacts is None:
            raise ValueError("lobes=True needs contacts=K")
        want_centrelines = centrelines is not None and centrelines is not False
        if want_centrelines and contacts is None:
            raise ValueError("centrelines=True needs contacts=K")
        if matches is not None and contacts is None:
            raise ValueError("matches=dict(bank=..., ...) needs contacts=K")
        if matches is not None and "bank" not in matches:
            raise ValueError("matches=dict(...) needs bank=, a match.TemplateBank")
        if textures is not None and contacts is None:
            raise ValueError("textures=dict(...) needs contacts=K")
        if outlines and contacts is None:
            raise ValueError("outlines=True needs contacts=K")
        if motion is not None and contacts is None:
            raise ValueError("motion=dict(...) needs contacts=K")
        if shapes and contacts is None:
            raise ValueError("shapes=True needs contacts=K")
        if thermal is not None and contacts is None:
            raise ValueError("thermal=temperature_crop needs contacts=K")
        o = self.predict_batch(image, format=format)
        torch.cuda.synchronize(self.device)
        status = int(o["status"][0].item())
        if status == _lib.FRAME_EMPTY_RELIABLE:
            return None
        if status != _lib.FRAME_OK:
            raise RuntimeError(f"frame failed with status {status}")
        s = o["scalars"][0].cpu().numpy()
        roi = self.intermediate("roi", 1, torch.uint8).view(self.h, self.w).cpu().numpy().astype(bool)
        res = {
            "height_map_mm_crop": o["height_map_mm"][0].cpu().numpy(),
            "roi_eroded_crop": roi,
            "output_reliable_crop": o["output_reliable"][0].cpu().numpy().astype(bool),
            "estimated_grating_period_px": float(s[5]),
        }
        for i, name in enumerate(SCALAR_NAMES[:-1]):
            if name not in res:
                res[name] = float(s[i])
        res["argmax_depth_index"] = int(s[4])
        res["argmin_unitless_index"] = int(s[8])
        if contacts is not None:
            from .writers import contacts_table, shapes_table
            c = self.shapes(int(contacts)) if shapes else self.contacts(int(contacts))
            rows = contacts_table(c["contacts"].cpu().numpy(), c["count"].cpu().numpy())
            for r in rows:
                r.pop("frame")
                r["centroid_xy"] = (r["centroid_x"], r["centroid_y"])
                r["argmax_xy"] = (r["argmax_index"] % self.w, r["argmax_index"] // self.w)
                r["bbox"] = (r["bbox_x0"], r["bbox_y0"], r["bbox_x1"], r["bbox_y1"])
            res["contacts"] = rows
            res["contact_count"] = int(c["count"][0].item())
            if shapes:
                res["shapes"] = shapes_table(c["shapes"].cpu().numpy(), c["contacts"].cpu().numpy(), c["count"].cpu().numpy())
                for r in res["shapes"]:
                    r.pop("frame")
            if thermal is not None:
                from .writers import thermal_frame_record, thermal_table
                crop = torch.as_tensor(thermal)
                t = self.thermal(crop[None] if crop.dim() == 2 else crop, int(contacts))
                res["thermal"] = thermal_table(t["thermal"].cpu().numpy(), t["contacts"].cpu().numpy(), t["count"].cpu().numpy())
                for r in res["thermal"]:
                    r.pop("frame")
                res["thermal_frame"] = thermal_frame_record(t["thermal_frame"][0].cpu().numpy())
            if motion is not None:
                from .writers import motion_frame_record, motion_table, tracks_table
                mo = self.motion(**dict(motion, max_contacts=int(contacts)))
                tab, cnt = mo["contacts"].cpu().numpy(), mo["count"].cpu().numpy()
                res["tracks"] = tracks_table(mo["tracks"].cpu().numpy(), tab, cnt)
                res["motion"] = motion_table(mo["motion"].cpu().numpy(), tab, cnt)
                for r in res["tracks"] + res["motion"]:
                    r.pop("frame")
                res["motion_frame"] = motion_frame_record(mo["motion_frame"][0].cpu().numpy())
            if outlines:
                from .writers import outline_frame_record, outlines_table
                ol = self.outlines(int(contacts))
                res["outlines"] = outlines_table(ol["outlines"].cpu().numpy(), ol["count"].cpu().numpy())
                for r in res["outlines"]:
                    r.pop("frame")
                res["outline_polylines"] = outline_frame_record(ol["outlines"][0].cpu().numpy(), ol["vertices"][0].cpu().numpy(),
                                                                ol["offsets"][0].cpu().numpy(), int(ol["count"][0].item()))["polylines"]
            if textures is not None:
                from .writers import textures_table
                tx = self.textures(int(contacts), **dict(textures))
                res["textures"] = textures_table(tx["textures"].cpu().numpy(), tx["count"].cpu().numpy())
                for r in res["textures"]:
                    r.pop("frame")
            if matches is not None:
                from .writers import matches_table
                mt = self.matches(max_contacts=int(contacts), **dict(matches))
                res["matches"] = matches_table(mt["matches"].cpu().numpy(), mt["count"].cpu().numpy())
                for r in res["matches"]:
                    r.pop("frame")
            if want_centrelines:
                from .writers import centreline_frame_record, centrelines_table
                cl = self.centrelines(int(contacts), skeleton=False, **({} if centrelines is True else dict(centrelines)))
                res["centrelines"] = centrelines_table(cl["centrelines"].cpu().numpy(), cl["count"].cpu().numpy())
                for r in res["centrelines"]:
                    r.pop("frame")
                if "stations" in cl:
                    rec = centreline_frame_record(cl["centrelines"][0].cpu().numpy(), cl["stations"][0].cpu().numpy(), cl["station_d2"][0].cpu().numpy(),
                                                  cl["offsets"][0].cpu().numpy(), int(cl["count"][0].item()))
                    res["centreline_stations"], res["centreline_d2"] = rec["stations"], rec["d2"]
                else:                                           # max_stations=0: no polylines were asked for
                    res["centreline_stations"], res["centreline_d2"] = [None] * len(res["centrelines"]), [None] * len(res["centrelines"])
            if want_lobes:
                from .writers import lobe_frame_record
                lb = self.lobes(int(contacts), split=True, **({} if lobes is True else dict(lobes)))
                rec = lobe_frame_record(lb["lobes"][0].cpu().numpy(), lb["lobe_rows"][0].cpu().numpy(), int(lb["count"][0].item()),
                                        lb["split_contacts"][0].cpu().numpy(), int(lb["split_count"][0].item()), lb["split_parent"][0].cpu().numpy())
                res["lobes"], res["lobe_rows"], res["split_contacts"] = rec["lobes"], rec["lobe_rows"], rec["split_contacts"]
        if pressure is not None:
            from .writers import pressure_frame_record, pressure_table
            running = self._pressure                            # without contacts=K the table's size is nobody's concern: keep the running one
            pr = self.pressure(**dict(pressure, max_contacts=int(contacts) if contacts is not None else (running.max_contacts if running else 8)))
            res["pressure_kpa"] = pr["pressure_kpa"][0].cpu().numpy()
            res["pressure_frame"] = pressure_frame_record(pr["pressure_frame"][0].cpu().numpy())
            if contacts is not None:
                res["pressure"] = pressure_table(pr["pressure"].cpu().numpy(), pr["count"].cpu().numpy())
                for r in res["pressure"]:
                    r.pop("frame")
        if taxels is not None:
            from .writers import taxel_frame_record
            t = self.taxels(taxels)
            res["taxels"] = t["taxels"][0].cpu().numpy()
            res["taxel_frame"] = taxel_frame_record(t["frame"][0].cpu().numpy())
        if temporal is not None:
            from .writers import temporal_frame_record
            res["temporal_frame"] = temporal_frame_record(self.temporal(**dict(temporal, planes=False))["frames"][0].cpu().numpy())
        if cloud is not None:
            from .writers import cloud_frame_record
            raw = self.cloud(**cloud)
            c = self._cloud.trim(raw)
            res["cloud"] = c["points"].cpu().numpy()
            res["cloud_pixel"] = c["pixel"].cpu().numpy()
            if "label" in c:
                res["cloud_label"] = c["label"].cpu().numpy()
            res["cloud_frame"] = cloud_frame_record(c["frame"][0].cpu().numpy())
        return res


_default_sensor: Optional[FtpSensor] = None


def predict(image, reference=None, taxels=None, format=None, **kwargs) -> Optional[Dict[str, Any]]:
    """predict(image[, reference]) -> force map dict.  With `reference` (and, the first time, the keyword
    arguments of FtpSensor) a session is (re)built; later calls reuse it.  taxels=layout adds the "taxels" and
    "taxel_frame" keys of `FtpSensor.predict`.  format: the layout of `image` and of `reference` (`FtpSensor.predict_batch`)."""
    global _default_sensor
    if reference is not None or _default_sensor is None:
        if reference is None:
            raise RuntimeError("predict() needs a reference frame on first use")
        if _default_sensor is not None:
            _default_sensor.close()
        kwargs.setdefault("max_batch", 1)
        _default_sensor = FtpSensor(reference, format=format, **kwargs)
    return _default_sensor.predict(image, taxels=taxels, format=format)
