"""Pressure read-out (include/vistaf_pressure.h): the contact pressure map an elastic skin carries under a depth plane.

An extension with no counterpart in the reference.  The force of a frame is one scalar, and the taxel read-out spreads it in proportion to
indentation (a Winkler foundation).  `PressureReadout.measure` gives, on the device, the normal traction linear elasticity assigns to the
depth plane for a layer of modulus `E_mpa`, Poisson's ratio `nu` and thickness `thickness_mm` bonded to a rigid base (math.inf: a
half-space) -- p^ = G(|k|) u^ in the Fourier domain, four float64 contractions on the matrix cores -- and per-contact and per-frame
tables: model load, tensile part, share of the calibrated force, mean and peak pressure, centre of pressure, edge share, and the modulus
the calibrated force implies.  The material constants are the caller's: the package holds no material data.  The definition is in the
header.  PyTorch is used only for device memory and streams.
"""
from __future__ import annotations

import ctypes
import math
from typing import Dict

import torch

from . import _lib
from ._handle import Handle, ptr

PRESSURE_NAMES = _lib.PRESSURE_NAMES
PRESSURE_FRAME_NAMES = _lib.PRESSURE_FRAME_NAMES


def _check_model(max_contacts: int, pad_px: int, E_mpa: float, nu: float, thickness_mm: float):
    if not 0 <= max_contacts <= _lib.MAX_CONTACTS:
        raise ValueError(f"max_contacts must be 0..{_lib.MAX_CONTACTS}")
    if not 0 <= pad_px <= 4096:
        raise ValueError("pad_px must be 0..4096")
    if not (math.isfinite(E_mpa) and E_mpa > 0.0):
        raise ValueError("E_mpa must be finite and > 0")
    if not 0.0 <= nu <= 0.49:
        raise ValueError("nu must be 0..0.49")
    if not thickness_mm > 0.0:
        raise ValueError("thickness_mm must be > 0 or math.inf")


class PressureReadout(Handle):
    """A pressure read-out for h x w planes, at most `max_batch` frames per call, tables of `max_contacts` rows (the K of the
    `FtpSensor.contacts` that feeds it; 0: the plane and the frame row only).  The depth plane is zero-filled to (h + pad_px) x (w + pad_px)
    before the transform, which is what keeps the periodic images of a contact away from it."""
    _destroy = "vistaf_pressure_destroy"

    def __init__(self, h: int, w: int, max_batch: int, max_contacts: int = 8, pad_px: int = 32, E_mpa: float = 1.0, nu: float = 0.45,
                 thickness_mm: float = math.inf, device="cuda:0"):
        self.h, self.w, self.max_batch, self.max_contacts, self.pad_px = int(h), int(w), int(max_batch), int(max_contacts), int(pad_px)
        self.E_mpa, self.nu, self.thickness_mm = float(E_mpa), float(nu), float(thickness_mm)
        _check_model(self.max_contacts, self.pad_px, self.E_mpa, self.nu, self.thickness_mm)
        self._open(device)
        self._call("vistaf_pressure_create", self.h, self.w, self.max_batch, self.max_contacts, self.pad_px, self.E_mpa, self.nu, self.thickness_mm,
                   ctypes.byref(self._h))

    def measure(self, depth_mm, mm_per_px, depth_eps_mm: float, contact_index=None, contacts=None, count=None, force_N=None,
                status=None) -> Dict[str, torch.Tensor]:
        """depth_mm [B,h,w] float32 (the height map of a predict), mm_per_px [B] float64; with max_contacts > 0 contact_index [B,h,w] int8,
        contacts [B,K,16] float64 and count [B] int32 as `FtpSensor.contacts(K, index_plane=True)` returns them; force_N [B] float64 and
        status [B] int32 are optional (device or host).  Returns device tensors: pressure_kpa [B,h,w] f32, frame [B,12] f64 (fields
        PRESSURE_FRAME_NAMES) and, with max_contacts > 0, rows [B,K,16] f64 (fields PRESSURE_NAMES, unused rows and fields NaN).  A frame
        whose status is not 0 has a zero plane and NaN rows."""
        dep = self._t(depth_mm, torch.float32, (None, self.h, self.w), f"depth_mm must be [B,{self.h},{self.w}]")
        b, k = int(dep.shape[0]), self.max_contacts
        if not 1 <= b <= self.max_batch:
            raise ValueError(f"batch {b} outside 1..max_batch {self.max_batch}")
        mpp = self._t(mm_per_px, torch.float64, (b,), "mm_per_px must be [B] for the B frames of depth_mm")
        if not math.isfinite(float(depth_eps_mm)):
            raise ValueError("depth_eps_mm must be finite")
        given = [a is not None for a in (contact_index, contacts, count)]
        if any(given) != all(given) or all(given) != (k > 0):
            raise ValueError("contact_index, contacts and count go together, and with max_contacts > 0 only")
        idx = tab = cnt = None
        if k > 0:
            msg = f"contact_index must be [B,{self.h},{self.w}], contacts [B,{k},{_lib.NCONTACT}] and count [B]"
            idx, tab = self._t(contact_index, torch.int8, dep.shape, msg), self._t(contacts, torch.float64, (b, k, _lib.NCONTACT), msg)
            cnt = self._t(count, torch.int32, (b,), msg)
        msg = "force_N and status must be [B] for the B frames of depth_mm"
        frc, sta = self._t(force_N, torch.float64, (b,), msg), self._t(status, torch.int32, (b,), msg)
        out = {"pressure_kpa": torch.empty((b, self.h, self.w), dtype=torch.float32, device=self.device),
               "frame": torch.empty((b, _lib.NPRESSUREFRAME), dtype=torch.float64, device=self.device)}
        if k > 0:
            out["rows"] = torch.empty((b, k, _lib.NPRESSURE), dtype=torch.float64, device=self.device)
        self._call("vistaf_pressure_measure", self._h, dep.data_ptr(), ptr(idx), ptr(tab), ptr(cnt), mpp.data_ptr(), ptr(frc), ptr(sta),
                   float(depth_eps_mm), b, out["pressure_kpa"].data_ptr(), ptr(out.get("rows")), out["frame"].data_ptr(), self._stream())
        return out
