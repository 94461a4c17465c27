"""Thermal read-out (include/vistaf_thermal.h): the temperature of each contact, via the alignment warp.

An extension with no counterpart in the reference.  The depth map and every table read out of it live in the aligned ROI crop; the
temperature map of `TempSensor.predict` lives in the photograph's frame.  `ThermalReadout.register` resamples the map into the crop with the
record `FtpAligner.align` returned (shift, crop origin, ECC warp), on the device; `ThermalReadout.measure` reduces the registered plane over
the rows of the contacts table -- temperature under each contact, of the skin around it, their contrast -- and to a frame record.  The
definition is in the header.  The temperature chain itself is parity-unpinned; the read-out inherits that and adds nothing to it.
PyTorch is used only for device memory and streams.
"""
from __future__ import annotations

import ctypes
import math

import torch

from . import _lib
from ._handle import Handle, ptr

THERMAL_NAMES = _lib.THERMAL_NAMES
THERMAL_FRAME_NAMES = _lib.THERMAL_FRAME_NAMES


class ThermalReadout(Handle):
    """A thermal read-out for h x w crops of H x W photographs cropped at `crop_origin` = (x1, y1), at most `max_batch` frames per call,
    tables of `max_contacts` rows (the K of the `FtpSensor.contacts` call that feeds it).  `apply_global_shift` is the aligner's flag: whether
    the recorded shift was applied to the photograph.  The surround of a contact is its box grown by `surround_margin_px`."""
    _destroy = "vistaf_thermal_destroy"

    def __init__(self, h: int, w: int, H: int, W: int, crop_origin=(0, 0), apply_global_shift: bool = True, max_batch: int = 1,
                 max_contacts: int = 8, surround_margin_px: int = 8, device="cuda:0"):
        self.h, self.w, self.H, self.W = int(h), int(w), int(H), int(W)
        self.crop_origin = (int(crop_origin[0]), int(crop_origin[1]))
        self.apply_global_shift = bool(apply_global_shift)
        self.max_batch, self.max_contacts, self.surround_margin_px = int(max_batch), int(max_contacts), int(surround_margin_px)
        if not 1 <= self.max_contacts <= _lib.MAX_CONTACTS:
            raise ValueError(f"max_contacts must be 1..{_lib.MAX_CONTACTS}")
        if not 0 <= self.surround_margin_px <= 4096:
            raise ValueError("surround_margin_px must be 0..4096")
        self._open(device)
        self._call("vistaf_thermal_create", self.h, self.w, self.H, self.W, *self.crop_origin, int(self.apply_global_shift), self.max_batch,
                   self.max_contacts, self.surround_margin_px, ctypes.byref(self._h), on_device=False)

    @classmethod
    def from_aligner(cls, aligner, max_batch=None, max_contacts: int = 8, surround_margin_px: int = 8):
        """The read-out of an `FtpAligner`'s crops: sizes, crop origin, shift flag and device are the aligner's."""
        return cls(*aligner.crop_shape, aligner.H, aligner.W, aligner.crop_box[:2], aligner.apply_global_shift,
                   aligner.max_batch if max_batch is None else max_batch, max_contacts, surround_margin_px, device=aligner.device)

    def register(self, temperature_map_C, align_info=None) -> torch.Tensor:
        """temperature_map_C [B,H,W] (or [H,W]) float32 in the photograph's frame, NaN where it has no value (`TempSensor.predict`);
        align_info [B,12] float64 as `FtpAligner.align` returns it under "info" (device or host), or None: no shift, identity warp.
        Returns the device tensor [B,h,w] f32: the map in the aligned crop's frame, NaN where the source lies outside the photograph."""
        t = torch.as_tensor(temperature_map_C)
        if t.dim() == 2:
            t = t[None]
        t = self._t(t, torch.float32, (None, self.H, self.W), f"temperature_map_C must be [B,{self.H},{self.W}]")
        b = int(t.shape[0])
        info = self._t(align_info, torch.float64, (b, _lib.ALIGN_NINFO), f"align_info must be [B,{_lib.ALIGN_NINFO}] for the B frames of temperature_map_C")
        if not 1 <= b <= self.max_batch:
            raise ValueError(f"batch {b} outside 1..max_batch {self.max_batch}")
        out = torch.empty((b, self.h, self.w), dtype=torch.float32, device=self.device)
        self._call("vistaf_thermal_register", self._h, t.data_ptr(), ptr(info), b, out.data_ptr(), self._stream())
        return out

    def measure(self, temp_crop, depth_mm, contact_index, contacts, count, depth_eps_mm: float, status=None):
        """temp_crop [B,h,w] float32 (`register`), depth_mm [B,h,w] float32 (the height map of a predict), contact_index [B,h,w] int8, contacts
        [B,K,16] float64 and count [B] int32 as `FtpSensor.contacts(K, index_plane=True)` returns them, status [B] int32 or None (every frame
        OK).  Returns device tensors {"thermal": [B,K,16] f64 (fields THERMAL_NAMES, unused rows and fields NaN), "frame": [B,8] f64 (fields
        THERMAL_FRAME_NAMES)}; a frame whose status is not 0 has NaN rows."""
        msg = f"temp_crop, depth_mm and contact_index must be [B,{self.h},{self.w}]"
        idx = self._t(contact_index, torch.int8, (None, self.h, self.w), msg)
        tmp, dep = self._t(temp_crop, torch.float32, idx.shape, msg), self._t(depth_mm, torch.float32, idx.shape, msg)
        b = int(idx.shape[0])
        msg = f"contacts must be [B,{self.max_contacts},{_lib.NCONTACT}] and count [B] for the B frames of contact_index"
        tab, cnt = self._t(contacts, torch.float64, (b, self.max_contacts, _lib.NCONTACT), msg), self._t(count, torch.int32, (b,), msg)
        st = self._t(status, torch.int32, (b,), "status must be [B] for the B frames of contact_index")
        if not 1 <= b <= self.max_batch:
            raise ValueError(f"batch {b} outside 1..max_batch {self.max_batch}")
        if not math.isfinite(float(depth_eps_mm)):
            raise ValueError("depth_eps_mm must be finite")
        out = {"thermal": torch.empty((b, self.max_contacts, _lib.NTHERMAL), dtype=torch.float64, device=self.device),
               "frame": torch.empty((b, _lib.NTHERMALFRAME), dtype=torch.float64, device=self.device)}
        self._call("vistaf_thermal_measure", self._h, tmp.data_ptr(), dep.data_ptr(), idx.data_ptr(), tab.data_ptr(), cnt.data_ptr(), ptr(st),
                   float(depth_eps_mm), b, out["thermal"].data_ptr(), out["frame"].data_ptr(), self._stream())
        return out
