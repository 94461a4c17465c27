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
from ._handle import Handle

SHAPE_NAMES = _lib.SHAPE_NAMES
SHAPE_FIT = _lib.SHAPE_FIT


class ContactShapes(Handle):
    """A shape read-out for h x w planes, at most `max_batch` frames per call, tables of `max_contacts` rows (the K of the
    `FtpSensor.contacts` call that feeds it).  The cap is fitted to the contact pixels at least `fit_min_fraction` of the contact's peak
    deep (0: every contact pixel)."""
    _destroy = "vistaf_shape_destroy"

    def __init__(self, h: int, w: int, max_batch: int, max_contacts: int = 8, fit_min_fraction: float = 0.5, device="cuda:0"):
        self.h, self.w, self.max_batch, self.max_contacts = int(h), int(w), int(max_batch), int(max_contacts)
        self.fit_min_fraction = float(fit_min_fraction)
        if not 1 <= self.max_contacts <= _lib.MAX_CONTACTS:
            raise ValueError(f"max_contacts must be 1..{_lib.MAX_CONTACTS}")
        if not 0.0 <= self.fit_min_fraction < 1.0:
            raise ValueError("fit_min_fraction must be in [0, 1)")
        self._open(device)
        self._call("vistaf_shape_create", self.h, self.w, self.max_batch, self.max_contacts, self.fit_min_fraction, ctypes.byref(self._h))

    def measure(self, depth_mm, contact_index, contacts, count, mm_per_px, depth_eps_mm: float) -> torch.Tensor:
        """depth_mm [B,h,w] float32 (the height map of a predict), contact_index [B,h,w] int8, contacts [B,K,16] float64 and count [B] int32
        as `FtpSensor.contacts(K, index_plane=True)` returns them, mm_per_px [B] float64 (device or host).  Returns the device tensor
        shapes [B,K,24] f64: fields SHAPE_NAMES, unused rows and fields NaN."""
        msg = f"depth_mm and contact_index must be [B,{self.h},{self.w}]"
        idx = self._t(contact_index, torch.int8, (None, self.h, self.w), msg)
        dep = self._t(depth_mm, torch.float32, idx.shape, msg)
        b = int(idx.shape[0])
        msg = f"contacts must be [B,{self.max_contacts},{_lib.NCONTACT}], count and mm_per_px [B] for the B frames of contact_index"
        tab = self._t(contacts, torch.float64, (b, self.max_contacts, _lib.NCONTACT), msg)
        cnt, mpp = self._t(count, torch.int32, (b,), msg), self._t(mm_per_px, torch.float64, (b,), msg)
        if not 1 <= b <= self.max_batch:
            raise ValueError(f"batch {b} outside 1..max_batch {self.max_batch}")
        if not math.isfinite(float(depth_eps_mm)):
            raise ValueError("depth_eps_mm must be finite")
        out = torch.empty((b, self.max_contacts, _lib.NSHAPE), dtype=torch.float64, device=self.device)
        self._call("vistaf_shape_measure", self._h, dep.data_ptr(), idx.data_ptr(), tab.data_ptr(), cnt.data_ptr(), mpp.data_ptr(),
                   float(depth_eps_mm), b, out.data_ptr(), self._stream())
        return out
