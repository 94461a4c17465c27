"""Contact motion read-out (include/vistaf_motion.h): slide, twist and lift of every tracked contact between consecutive frames.

An extension with no counterpart in the reference.  `FtpSensor.track` says which touch of the frame before a contact continues;
`ContactMotion.update` registers, on the device, the depth surface that parent left onto the current depth plane and gives the rigid
in-plane motion (tx, ty, theta) and the uniform depth change beta of every linked contact, with their standard errors.  The definition is
in the header.  PyTorch is used only for device memory and streams.
"""
from __future__ import annotations

import ctypes
import math
from typing import Dict

import torch

from . import _lib
from ._handle import Handle

MOTION_NAMES = _lib.MOTION_NAMES
MOTION_FRAME_NAMES = _lib.MOTION_FRAME_NAMES
MOTION_STATUS = _lib.MOTION_STATUS


class ContactMotion(Handle):
    """A motion read-out for h x w planes, at most `max_batch` frames per update, tables of `max_contacts` rows (the K of the
    `FtpSensor.contacts` and `ContactTracker` that feed it).  Every linked contact is registered with exactly `iterations` (1..16)
    Gauss-Newton steps; its status is ok when the last step is at most `tol_px`.  A parent with fewer than `min_pixels` contact pixels is
    not registered.  init_from_centroid starts the translation at the tracker's (dx, dy), else at 0.  Frames of one update are consecutive
    in time, and frame 0 of an update follows the last frame of the update before it: the read-out keeps that frame on the device until
    `reset()`.  It must see the same sequence of frames as the tracker whose rows it is handed."""
    _destroy = "vistaf_motion_destroy"

    def __init__(self, h: int, w: int, max_batch: int, max_contacts: int = 8, iterations: int = 8, tol_px: float = 1e-3, min_pixels: int = 16,
                 init_from_centroid: bool = True, device="cuda:0"):
        self.h, self.w, self.max_batch, self.max_contacts = int(h), int(w), int(max_batch), int(max_contacts)
        self.iterations, self.tol_px, self.min_pixels = int(iterations), float(tol_px), int(min_pixels)
        self.init_from_centroid = bool(init_from_centroid)
        if not 1 <= self.max_contacts <= _lib.MAX_CONTACTS:
            raise ValueError(f"max_contacts must be 1..{_lib.MAX_CONTACTS}")
        if not 1 <= self.iterations <= 16:
            raise ValueError("iterations must be 1..16")
        if not (math.isfinite(self.tol_px) and self.tol_px >= 0.0):
            raise ValueError("tol_px must be finite and >= 0")
        if self.min_pixels < 1:
            raise ValueError("min_pixels must be >= 1")
        self._open(device)
        self._call("vistaf_motion_create", self.h, self.w, self.max_batch, self.max_contacts, self.iterations, self.tol_px, self.min_pixels,
                   int(self.init_from_centroid), ctypes.byref(self._h))

    def update(self, depth_mm, contact_index, contacts, count, tracks, mm_per_px, depth_eps_mm: float) -> Dict[str, torch.Tensor]:
        """depth_mm [B,h,w] float32 (the height map of a predict), contact_index [B,h,w] int8, contacts [B,K,16] float64 and count [B] int32
        as `FtpSensor.contacts(K, index_plane=True)` returns them, tracks [B,K,16] float64 as `ContactTracker.update` returns it for the
        same frames, mm_per_px [B] float64 (device or host).  Returns device tensors: motion [B,K,24] f64 (fields MOTION_NAMES, unused rows
        and fields NaN) and frame [B,8] f64 (fields MOTION_FRAME_NAMES; all NaN for a frame without contacts)."""
        msg = f"depth_mm and contact_index must be [B,{self.h},{self.w}]"
        idx = self._t(contact_index, torch.int8, (None, self.h, self.w), msg)
        dep = self._t(depth_mm, torch.float32, idx.shape, msg)
        b, k = int(idx.shape[0]), self.max_contacts
        msg = f"contacts must be [B,{k},{_lib.NCONTACT}] and tracks [B,{k},{_lib.NTRACK}] for the B frames of contact_index"
        tab, trk = self._t(contacts, torch.float64, (b, k, _lib.NCONTACT), msg), self._t(tracks, torch.float64, (b, k, _lib.NTRACK), msg)
        msg = "count and mm_per_px must be [B] for the B frames of contact_index"
        cnt, mpp = self._t(count, torch.int32, (b,), msg), self._t(mm_per_px, torch.float64, (b,), msg)
        if not 1 <= b <= self.max_batch:
            raise ValueError(f"batch {b} outside 1..max_batch {self.max_batch}")
        if not math.isfinite(float(depth_eps_mm)):
            raise ValueError("depth_eps_mm must be finite")
        out = {"motion": torch.empty((b, self.max_contacts, _lib.NMOTION), dtype=torch.float64, device=self.device),
               "motion_frame": torch.empty((b, _lib.NMOTIONFRAME), dtype=torch.float64, device=self.device)}
        self._call("vistaf_motion_update", self._h, dep.data_ptr(), idx.data_ptr(), tab.data_ptr(), cnt.data_ptr(), trk.data_ptr(), mpp.data_ptr(),
                   float(depth_eps_mm), b, out["motion"].data_ptr(), out["motion_frame"].data_ptr(), self._stream())
        return out

    def reset(self):
        """forget the carried frame: every contact of the next frame is without a parent"""
        self._call("vistaf_motion_reset", self._h, on_device=False)
