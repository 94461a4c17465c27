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

MOTION_NAMES = _lib.MOTION_NAMES
MOTION_FRAME_NAMES = _lib.MOTION_FRAME_NAMES
MOTION_STATUS = _lib.MOTION_STATUS


class ContactMotion:
    """A motion read-out for h x w planes, at most `max_batch` frames per update, tables of `max_contacts` rows (the K of the
    `FtpSensor.contacts` and `ContactTracker` that feed it).  Every linked contact is registered with exactly `iterations` (1..16)
    Gauss-Newton steps; its status is ok when the last step is at most `tol_px`.  A parent with fewer than `min_pixels` contact pixels is
    not registered.  init_from_centroid starts the translation at the tracker's (dx, dy), else at 0.  Frames of one update are consecutive
    in time, and frame 0 of an update follows the last frame of the update before it: the read-out keeps that frame on the device until
    `reset()`.  It must see the same sequence of frames as the tracker whose rows it is handed."""

    def __init__(self, h: int, w: int, max_batch: int, max_contacts: int = 8, iterations: int = 8, tol_px: float = 1e-3, min_pixels: int = 16,
                 init_from_centroid: bool = True, device="cuda:0"):
        self._lib = _lib.load()
        self._h = ctypes.c_void_p()
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
        if not torch.cuda.is_available():
            raise RuntimeError("ContactMotion needs a HIP device (torch.cuda.is_available() is False); there is no CPU path")
        self.device = torch.device(device)
        with torch.cuda.device(self.device):
            _lib.check(self._lib.vistaf_motion_create(self.h, self.w, self.max_batch, self.max_contacts, self.iterations, self.tol_px,
                                                      self.min_pixels, int(self.init_from_centroid), ctypes.byref(self._h)))

    def update(self, depth_mm, contact_index, contacts, count, tracks, mm_per_px, depth_eps_mm: float) -> Dict[str, torch.Tensor]:
        """depth_mm [B,h,w] float32 (the height map of a predict), contact_index [B,h,w] int8, contacts [B,K,16] float64 and count [B] int32
        as `FtpSensor.contacts(K, index_plane=True)` returns them, tracks [B,K,16] float64 as `ContactTracker.update` returns it for the
        same frames, mm_per_px [B] float64 (device or host).  Returns device tensors: motion [B,K,24] f64 (fields MOTION_NAMES, unused rows
        and fields NaN) and frame [B,8] f64 (fields MOTION_FRAME_NAMES; all NaN for a frame without contacts)."""
        dep = torch.as_tensor(depth_mm).to(self.device, torch.float32).contiguous()
        idx = torch.as_tensor(contact_index).to(self.device, torch.int8).contiguous()
        tab = torch.as_tensor(contacts).to(self.device, torch.float64).contiguous()
        cnt = torch.as_tensor(count).to(self.device, torch.int32).contiguous()
        trk = torch.as_tensor(tracks).to(self.device, torch.float64).contiguous()
        mpp = torch.as_tensor(mm_per_px).to(self.device, torch.float64).contiguous()
        if idx.dim() != 3 or tuple(idx.shape[1:]) != (self.h, self.w) or tuple(dep.shape) != tuple(idx.shape):
            raise ValueError(f"depth_mm and contact_index must be [B,{self.h},{self.w}]")
        b = int(idx.shape[0])
        if tuple(tab.shape) != (b, self.max_contacts, _lib.NCONTACT) or tuple(trk.shape) != (b, self.max_contacts, _lib.NTRACK):
            raise ValueError(f"contacts must be [B,{self.max_contacts},{_lib.NCONTACT}] and tracks [B,{self.max_contacts},{_lib.NTRACK}] for the B "
                             "frames of contact_index")
        if tuple(cnt.shape) != (b,) or tuple(mpp.shape) != (b,):
            raise ValueError("count and mm_per_px must be [B] for the B frames of contact_index")
        if not 1 <= b <= self.max_batch:
            raise ValueError(f"batch {b} outside 1..max_batch {self.max_batch}")
        if not math.isfinite(float(depth_eps_mm)):
            raise ValueError("depth_eps_mm must be finite")
        out = {"motion": torch.empty((b, self.max_contacts, _lib.NMOTION), dtype=torch.float64, device=self.device),
               "motion_frame": torch.empty((b, _lib.NMOTIONFRAME), dtype=torch.float64, device=self.device)}
        with torch.cuda.device(self.device):
            _lib.check(self._lib.vistaf_motion_update(self._h, dep.data_ptr(), idx.data_ptr(), tab.data_ptr(), cnt.data_ptr(), trk.data_ptr(),
                                                      mpp.data_ptr(), float(depth_eps_mm), b, out["motion"].data_ptr(),
                                                      out["motion_frame"].data_ptr(), int(torch.cuda.current_stream(self.device).cuda_stream)))
        return out

    def reset(self):
        """forget the carried frame: every contact of the next frame is without a parent"""
        _lib.check(self._lib.vistaf_motion_reset(self._h))

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            self._lib.vistaf_motion_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
