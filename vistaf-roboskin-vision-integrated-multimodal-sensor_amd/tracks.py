"""Contact tracker (include/vistaf_track.h): persistent ids, motion, split and merge of the contacts of consecutive frames.

An extension with no counterpart in the reference.  `FtpSensor.contacts(K, index_plane=True)` gives one table per frame whose rows are
ordered by peak depth; `ContactTracker.update` links the rows of consecutive frames on the device, from those index planes and tables, so
nothing is copied to the host to follow a touch through time.  The definition of the link is in the header.  PyTorch is used only for
device memory and streams.
"""
from __future__ import annotations

import ctypes
import math
from typing import Dict

import torch

from . import _lib
from ._handle import Handle

TRACK_NAMES = _lib.TRACK_NAMES
TRACK_EVENTS = _lib.TRACK_EVENTS


class ContactTracker(Handle):
    """A tracker for h x w index planes, at most `max_batch` frames per update, tables of `max_contacts` rows (the K of the
    `FtpSensor.contacts` calls that feed it).  gate_px > 0 adds the gate stage: contacts without any overlap are linked when their centroids
    are no further apart than gate_px, nearest pair first.  Frames of one update are consecutive in time, and frame 0 of an update follows
    the last frame of the update before it: the tracker keeps that frame on the device until `reset()`."""
    _destroy = "vistaf_track_destroy"

    def __init__(self, h: int, w: int, max_batch: int, max_contacts: int = 8, gate_px: float = 0.0, device="cuda:0"):
        self.h, self.w, self.max_batch, self.max_contacts, self.gate_px = int(h), int(w), int(max_batch), int(max_contacts), float(gate_px)
        if not 1 <= self.max_contacts <= _lib.MAX_CONTACTS:
            raise ValueError(f"max_contacts must be 1..{_lib.MAX_CONTACTS}")
        if not (math.isfinite(self.gate_px) and self.gate_px >= 0.0):
            raise ValueError("gate_px must be finite and >= 0")
        self._open(device)
        self._call("vistaf_track_create", self.h, self.w, self.max_batch, self.max_contacts, self.gate_px, ctypes.byref(self._h))

    def update(self, contact_index, contacts, count) -> Dict[str, torch.Tensor]:
        """contact_index [B,h,w] int8, contacts [B,K,16] float64, count [B] int32, as `FtpSensor.contacts(K, index_plane=True)` returns them
        (device or host).  Returns device tensors: tracks [B,K,16] f64 (fields TRACK_NAMES, unused rows and fields NaN) and fate [B,K] i32
        (what became of row i of the frame before: the continuing row, -1 ended, -(2 + j) absorbed into contact j, INT32_MIN no such row)."""
        idx = self._t(contact_index, torch.int8, (None, self.h, self.w), f"contact_index must be [B,{self.h},{self.w}]")
        b = int(idx.shape[0])
        msg = f"contacts must be [B,{self.max_contacts},{_lib.NCONTACT}] and count [B] for the B frames of contact_index"
        tab, cnt = self._t(contacts, torch.float64, (b, self.max_contacts, _lib.NCONTACT), msg), self._t(count, torch.int32, (b,), msg)
        if not 1 <= b <= self.max_batch:
            raise ValueError(f"batch {b} outside 1..max_batch {self.max_batch}")
        out = {"tracks": torch.empty((b, self.max_contacts, _lib.NTRACK), dtype=torch.float64, device=self.device),
               "fate": torch.empty((b, self.max_contacts), dtype=torch.int32, device=self.device)}
        self._call("vistaf_track_update", self._h, idx.data_ptr(), tab.data_ptr(), cnt.data_ptr(), b, out["tracks"].data_ptr(),
                   out["fate"].data_ptr(), self._stream())
        return out

    def reset(self):
        """forget the carried frame and restart ids at 0"""
        self._call("vistaf_track_reset", self._h, on_device=False)
