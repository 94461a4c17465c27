"""Temporal read-out (include/vistaf_temporal.h): filtered depth, rate, touch state and events of a stream of depth planes.

An extension with no counterpart in the reference.  The other read-outs describe one frame in isolation and the tracker links table rows;
a controller asks of every pixel whether it is touched now and since when, whether it is loading or unloading and how fast, whether a touch
began or ended in this frame, and what the depth map is without frame-to-frame flicker.  `TemporalReadout.update` answers on the device:
an exponential filter, its rate, a Schmitt trigger, the dwell of its bit and the peak raw depth of the running touch per pixel, carried
from call to call, and one row of 16 doubles per frame -- so no depth map is copied to the host to write a recurrence in NumPy.  The
definition is in the header.  PyTorch is used only for device memory and streams.
"""
from __future__ import annotations

import ctypes
from typing import Dict

import torch

from . import _lib
from ._handle import Handle, ptr

TEMPORAL_NAMES = _lib.TEMPORAL_NAMES
TEMPORAL_EVENTS = _lib.TEMPORAL_EVENTS


class TemporalReadout(Handle):
    """A temporal read-out for h x w planes, at most `max_batch` frames per update.  alpha in (0, 1] is the filter's weight of the new
    frame, on_mm > off_mm >= 0 the thresholds of the touch bit (each rounded once to float32), frame_period_s > 0 the fixed time between
    frames.  Frames of one update are consecutive in time, and frame 0 of an update follows the last frame of the update before it: the
    read-out keeps five state planes on the device until `reset()`.  Creating it needs no device, `update` and `state` do."""
    _destroy = "vistaf_temporal_destroy"

    def __init__(self, h: int, w: int, max_batch: int, alpha: float, on_mm: float, off_mm: float, frame_period_s: float, device="cuda:0"):
        self.h, self.w, self.max_batch = int(h), int(w), int(max_batch)
        self.alpha, self.on_mm, self.off_mm, self.frame_period_s = float(alpha), float(on_mm), float(off_mm), float(frame_period_s)
        self._open(device, need_device=False)
        self._call("vistaf_temporal_create", self.h, self.w, self.max_batch, self.alpha, self.on_mm, self.off_mm, self.frame_period_s,
                   ctypes.byref(self._h), on_device=False)

    def update(self, depth, mm_per_px, status=None, planes: bool = False) -> Dict[str, torch.Tensor]:
        """depth [B,h,w] float32 (the height map of a predict), mm_per_px [B] float64, status [B] int32 or None (every frame OK; a frame
        whose status is not 0 is skipped: it changes no state and its row is NaN but for gap_frames), device or host.  Returns the device
        tensor {"frames": [B,16] f64 (fields TEMPORAL_NAMES)} and, with planes=True, "filtered" [B,h,w] f32 and "touch" [B,h,w] u8, the
        state after every frame."""
        self._need_device("update")
        dep = self._t(depth, torch.float32, (None, self.h, self.w), f"depth must be [B,{self.h},{self.w}]")
        b = int(dep.shape[0])
        msg = "mm_per_px and status must be [B] for the B frames of depth"
        mpp, sta = self._t(mm_per_px, torch.float64, (b,), msg), self._t(status, torch.int32, (b,), msg)
        if not 1 <= b <= self.max_batch:
            raise ValueError(f"batch {b} outside 1..max_batch {self.max_batch}")
        out = {"frames": torch.empty((b, _lib.NTEMPORAL), dtype=torch.float64, device=self.device)}
        if planes:
            out["filtered"] = torch.empty((b, self.h, self.w), dtype=torch.float32, device=self.device)
            out["touch"] = torch.empty((b, self.h, self.w), dtype=torch.uint8, device=self.device)
        self._call("vistaf_temporal_update", self._h, dep.data_ptr(), mpp.data_ptr(), ptr(sta), b, out["frames"].data_ptr(),
                   out["filtered"].data_ptr() if planes else None, out["touch"].data_ptr() if planes else None, self._stream())
        return out

    def state(self) -> Dict[str, torch.Tensor]:
        """Copies of the five state planes [h,w] (device): filt f32, rate f32 (mm/s), touch u8, dwell i32 (accepted frames since the bit
        last changed), hold f32 (largest raw depth of the running touch)."""
        self._need_device("state")
        out = {"filt": torch.empty((self.h, self.w), dtype=torch.float32, device=self.device),
               "rate": torch.empty((self.h, self.w), dtype=torch.float32, device=self.device),
               "touch": torch.empty((self.h, self.w), dtype=torch.uint8, device=self.device),
               "dwell": torch.empty((self.h, self.w), dtype=torch.int32, device=self.device),
               "hold": torch.empty((self.h, self.w), dtype=torch.float32, device=self.device)}
        self._call("vistaf_temporal_state", self._h, out["filt"].data_ptr(), out["rate"].data_ptr(), out["touch"].data_ptr(), out["dwell"].data_ptr(),
                   out["hold"].data_ptr(), self._stream())
        return out

    def reset(self):
        """forget the stream: the next update starts from an untouched, unprimed state"""
        self._call("vistaf_temporal_reset", self._h, on_device=False)
