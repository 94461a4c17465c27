"""Per-contact shape read-out (include/vistaf_shape.h): footprint ellipse, boundary and cap curvature of every contact.

An extension with no counterpart in the reference.  `FtpSensor.contacts(K, index_plane=True)` says where a touch is and how strong;
`ContactShapes.measure` says what it looks like -- the axes and direction of its footprint, its boundary pixels, and the apex, curvatures
and radii of the quadric cap fitted to its depth -- on the device, from the height map, the index plane and the table, so no plane is
copied to the host to tell a ball from an edge.  The definition is in the header.  PyTorch is used only for device memory and streams.
"""
from __future__ import annotations

import ctypes
import math

import torch

from . import _lib

SHAPE_NAMES = _lib.SHAPE_NAMES
SHAPE_FIT = _lib.SHAPE_FIT


class ContactShapes:
    """A shape read-out for h x w planes, at most `max_batch` frames per call, tables of `max_contacts` rows (the K of the
    `FtpSensor.contacts` call that feeds it).  The cap is fitted to the contact pixels at least `fit_min_fraction` of the contact's peak
    deep (0: every contact pixel)."""

    def __init__(self, h: int, w: int, max_batch: int, max_contacts: int = 8, fit_min_fraction: float = 0.5, device="cuda:0"):
        self._lib = _lib.load()
        self._h = ctypes.c_void_p()
        self.h, self.w, self.max_batch, self.max_contacts = int(h), int(w), int(max_batch), int(max_contacts)
        self.fit_min_fraction = float(fit_min_fraction)
        if not 1 <= self.max_contacts <= _lib.MAX_CONTACTS:
            raise ValueError(f"max_contacts must be 1..{_lib.MAX_CONTACTS}")
        if not 0.0 <= self.fit_min_fraction < 1.0:
            raise ValueError("fit_min_fraction must be in [0, 1)")
        if not torch.cuda.is_available():
            raise RuntimeError("ContactShapes needs a HIP device (torch.cuda.is_available() is False); there is no CPU path")
        self.device = torch.device(device)
        with torch.cuda.device(self.device):
            _lib.check(self._lib.vistaf_shape_create(self.h, self.w, self.max_batch, self.max_contacts, self.fit_min_fraction,
                                                     ctypes.byref(self._h)))

    def measure(self, depth_mm, contact_index, contacts, count, mm_per_px, depth_eps_mm: float) -> torch.Tensor:
        """depth_mm [B,h,w] float32 (the height map of a predict), contact_index [B,h,w] int8, contacts [B,K,16] float64 and count [B] int32
        as `FtpSensor.contacts(K, index_plane=True)` returns them, mm_per_px [B] float64 (device or host).  Returns the device tensor
        shapes [B,K,24] f64: fields SHAPE_NAMES, unused rows and fields NaN."""
        dep = torch.as_tensor(depth_mm).to(self.device, torch.float32).contiguous()
        idx = torch.as_tensor(contact_index).to(self.device, torch.int8).contiguous()
        tab = torch.as_tensor(contacts).to(self.device, torch.float64).contiguous()
        cnt = torch.as_tensor(count).to(self.device, torch.int32).contiguous()
        mpp = torch.as_tensor(mm_per_px).to(self.device, torch.float64).contiguous()
        if idx.dim() != 3 or tuple(idx.shape[1:]) != (self.h, self.w) or tuple(dep.shape) != tuple(idx.shape):
            raise ValueError(f"depth_mm and contact_index must be [B,{self.h},{self.w}]")
        b = int(idx.shape[0])
        if tuple(tab.shape) != (b, self.max_contacts, _lib.NCONTACT) or tuple(cnt.shape) != (b,) or tuple(mpp.shape) != (b,):
            raise ValueError(f"contacts must be [B,{self.max_contacts},{_lib.NCONTACT}], count and mm_per_px [B] for the B frames of contact_index")
        if not 1 <= b <= self.max_batch:
            raise ValueError(f"batch {b} outside 1..max_batch {self.max_batch}")
        if not math.isfinite(float(depth_eps_mm)):
            raise ValueError("depth_eps_mm must be finite")
        out = torch.empty((b, self.max_contacts, _lib.NSHAPE), dtype=torch.float64, device=self.device)
        with torch.cuda.device(self.device):
            _lib.check(self._lib.vistaf_shape_measure(self._h, dep.data_ptr(), idx.data_ptr(), tab.data_ptr(), cnt.data_ptr(), mpp.data_ptr(),
                                                      float(depth_eps_mm), b, out.data_ptr(),
                                                      int(torch.cuda.current_stream(self.device).cuda_stream)))
        return out

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            self._lib.vistaf_shape_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
