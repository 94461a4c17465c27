"""Indenter match read-out (include_ext/vistaf_match.h): which known object touches, where on the skin and how it is turned.

An extension with no counterpart in the reference.  The other read-outs describe a touch; `contact_matches` recognises it: a `TemplateBank`
holds T depth imprints of known indenters (metric height maps, each with a class id and a rotational symmetry order), rotated, centred and
normalised once on the host, and for every row of the per-contact table the device samples a metric patch about the contact's centroid,
correlates every bank row with every shift of it on the matrix cores and reports the best template with its class, rotation and position, the
normalised score and the best score of another class, the amplitude and residual of the fit, and a label that is withheld when the match is
weak or ambiguous -- so the depth planes are not copied to the host to tell a ball from a screw head.  Four plain functions of the library and
no handle: the bank and the workspace are tensors of the caller's.  The definition is in the header.  PyTorch is used only for device memory
and streams.
"""
from __future__ import annotations

import ctypes
from typing import Dict, Optional

import numpy as np
import torch

from . import _lib
from ._handle import call, stream
from ._workspace import Workspace, table_inputs
from ._workspace import workspace_bytes as _workspace_bytes

MATCH_NAMES = _lib.MATCH_NAMES
MATCH_STATUS = _lib.MATCH_STATUS
MATCH_FLAGS = _lib.MATCH_FLAGS


def _i32(values):
    a = np.ascontiguousarray(np.asarray(values, dtype=np.int32).reshape(-1))
    return a, a.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))


def bank_bytes(T: int, P: int, R: int, symmetry) -> int:
    """the bytes of a bank of T templates of P x P over R rotation steps with these symmetry orders; ValueError for sizes the read-out does
    not take.  Needs no device."""
    sym, psym = _i32(symmetry)
    if sym.size != int(T):
        raise ValueError("symmetry must hold one order per template")
    n = ctypes.c_size_t()
    call(None, "vistaf_match_bank_bytes", int(T), int(P), int(R), psym, ctypes.byref(n))
    return int(n.value)


def workspace_bytes(h: int, w: int, max_batch: int, max_contacts: int, P: int, max_shift: int, M: int) -> int:
    """the bytes of the workspace `contact_matches` needs for up to max_batch frames of h x w, tables of max_contacts rows, a bank of M rows
    of P x P templates and shifts up to max_shift; ValueError for sizes the read-out does not take.  Needs no device."""
    return _workspace_bytes(MatchWorkspace._sizer, h, w, max_batch, max_contacts, P, max_shift, M)


class TemplateBank:
    """T imprints of known indenters, ready to be matched: templates [T,P,P] float32 mm (P odd, 5..33) sampled at template_mm_per_px, klass [T]
    their class ids (>= 0), symmetry [T] their rotational symmetry orders (0: a body of revolution, one rotation; n: searched over R/n of
    the R rotation steps, n dividing R).  The bank is built on the host by the library (`vistaf_match_build_bank`; ValueError for a flat
    template, naming its index) and is `host`, a uint8 array whose sections the properties below view; `device_bytes(device)` is the copy
    on a device, made once per device."""

    def __init__(self, templates, klass, symmetry, template_mm_per_px: float, rotations: int = 24):
        tp = np.ascontiguousarray(np.asarray(templates, dtype=np.float32))
        if tp.ndim != 3 or tp.shape[1] != tp.shape[2]:
            raise ValueError("templates must be [T,P,P]")
        self.T, self.P, self.R = int(tp.shape[0]), int(tp.shape[1]), int(rotations)
        kl, pkl = _i32(klass)
        sym, psym = _i32(symmetry)
        if kl.size != self.T or sym.size != self.T:
            raise ValueError("klass and symmetry must hold one entry per template")
        self.template_mm_per_px = float(template_mm_per_px)
        self.nbytes = bank_bytes(self.T, self.P, self.R, sym)
        self._raw = np.zeros((self.nbytes + 8,), dtype=np.uint8)
        skip = (-self._raw.ctypes.data) % 8
        self.host = self._raw[skip:skip + self.nbytes]
        call(None, "vistaf_match_build_bank", tp.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), pkl, psym, self.T, self.P, self.R,
             self.template_mm_per_px, self.host.ctypes.data, self.nbytes)
        self.header = self.host[:4 * _lib.MATCH_HEADER_INTS].view(np.int32)
        self.M, self.D, self.Dp = int(self.header[4]), int(self.header[5]), int(self.header[6])
        up = lambda v, a: (v + a - 1) // a * a
        o = self.offsets = {"cossin": 4 * _lib.MATCH_HEADER_INTS}
        o["rowtab"] = o["cossin"] + 16 * self.R
        o["klass"] = o["rowtab"] + 8 * self.M
        o["symmetry"] = o["klass"] + 4 * self.T
        o["disc"] = up(o["symmetry"] + 4 * self.T, 8)
        o["mu"] = o["disc"] + 8 * self.D
        o["norm"] = o["mu"] + 8 * self.M
        o["rows"] = up(o["norm"] + 8 * self.M, 256)
        o["end"] = o["rows"] + 8 * self.M * self.Dp
        self._device: Dict[str, torch.Tensor] = {}

    def _view(self, name, dtype, shape):
        n = int(np.prod(shape)) * np.dtype(dtype).itemsize
        return self.host[self.offsets[name]:self.offsets[name] + n].view(dtype).reshape(shape)

    cossin = property(lambda self: self._view("cossin", np.float64, (self.R, 2)))
    rowtab = property(lambda self: self._view("rowtab", np.int32, (self.M, 2)))
    klass = property(lambda self: self._view("klass", np.int32, (self.T,)))
    symmetry = property(lambda self: self._view("symmetry", np.int32, (self.T,)))
    disc = property(lambda self: self._view("disc", np.int32, (self.D, 2)))
    mu = property(lambda self: self._view("mu", np.float64, (self.M,)))
    norm = property(lambda self: self._view("norm", np.float64, (self.M,)))
    rows = property(lambda self: self._view("rows", np.float64, (self.M, self.Dp)))

    def device_bytes(self, device) -> torch.Tensor:
        """the bank's bytes on `device` (uint8, 256-byte aligned by the allocator), copied on first use"""
        key = str(torch.device(device))
        if key not in self._device:
            self._device[key] = torch.from_numpy(np.array(self.host, copy=True)).to(device)
        return self._device[key]


class MatchWorkspace(Workspace):
    """The device memory of the read-out for up to `batch` frames of h x w, tables of max_contacts rows, a bank of M rows of P x P templates
    and shifts up to max_shift: one tensor, nothing of the library's.  `close()` drops it."""

    _sizer = "vistaf_match_workspace_bytes"

    def __init__(self, h: int, w: int, batch: int, max_contacts: int, P: int, max_shift: int, M: int, device="cuda:0"):
        super().__init__(device, h, w, batch, max_contacts, P, max_shift, M)


def contact_matches(depth, contact_index, contacts, count, mm_per_px, eps: float, bank: TemplateBank, ws: Optional[MatchWorkspace] = None,
                    max_shift: int = 3, min_pixels: int = 6, accept_score: float = 0.7, accept_margin: float = 0.05,
                    device="cuda:0") -> Dict[str, torch.Tensor]:
    """depth [B,h,w] float32 (the height map of a predict), contact_index [B,h,w] int8, contacts [B,K,16] float64 and count [B] int32 as
    `FtpSensor.contacts(K, index_plane=True)` returns them, mm_per_px [B] float64 (device or host), eps the session's depth_eps_mm, bank a
    TemplateBank.  max_shift m in 0..8: the templates are tried at (2m+1)^2 positions about the contact's centroid, in template pixels;
    min_pixels: the least number of touching samples under the template for a position to count; accept_score, accept_margin: a match below
    that score is WEAK, one closer than that to the best template of another class AMBIGUOUS, and either withholds the label.  Returns
    device tensors: matches [B,K,24] f64 (fields MATCH_NAMES, unused rows NaN), scores [B,K,T] f64 (per template its best score) and patches
    [B,K,S,S] f32, S = P + 2m (the metric crop about each contact that was matched).  ws: a MatchWorkspace that fits, else one is made for
    the call."""
    dev, idx, tab, cnt, mpp, dep, b, h, w, k = table_inputs("contact_matches", contact_index, contacts, count, mm_per_px, device, depth,
                                                            "depth must be [B,h,w] as contact_index")
    if not isinstance(bank, TemplateBank):
        raise TypeError("bank must be a TemplateBank")
    m = int(max_shift)
    if not 0 <= m <= _lib.MATCH_MAX_SHIFT:
        raise ValueError(f"max_shift must be 0..{_lib.MATCH_MAX_SHIFT}")
    work = MatchWorkspace.fitting(ws, dev, h, w, b, k, bank.P, m, bank.M)
    s = bank.P + 2 * m
    res = {"matches": torch.empty((b, k, _lib.NMATCH), dtype=torch.float64, device=dev),
           "scores": torch.empty((b, k, bank.T), dtype=torch.float64, device=dev),
           "patches": torch.empty((b, k, s, s), dtype=torch.float32, device=dev)}
    dbank = bank.device_bytes(dev)
    call(dev, "vistaf_match_measure", dep.data_ptr(), idx.data_ptr(), tab.data_ptr(), cnt.data_ptr(), mpp.data_ptr(), dbank.data_ptr(), bank.nbytes,
         bank.header.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), float(eps), m, int(min_pixels), float(accept_score), float(accept_margin), h, w, b, k,
         res["matches"].data_ptr(), res["scores"].data_ptr(), res["patches"].data_ptr(), work.pointer(), work.nbytes, stream(dev))
    return res
