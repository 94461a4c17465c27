"""Point-cloud read-out (include/vistaf_cloud.h): the contact surface as metric points with a normal and curvature each.

An extension with no counterpart in the reference.  Every other read-out summarises the depth map; a grasp planner, a registration or pose
estimator or a point-cloud publisher wants the touched surface itself: points in millimetres with a unit normal each.  `CloudReadout.measure`
produces them on the device -- the surface pixels (depth > depth_eps_mm) of every frame of a batch, every stride-th column and row,
compacted in pixel order into records of 8 float32 (x, y, z, nx, ny, nz, mean and Gaussian curvature), the pixel and contact label of each
point, the frame offsets, and one row of 12 doubles per frame (areas, mean normal, tilt, steepest slope) -- so no depth map is copied to
the host to be thresholded, differentiated and compacted in NumPy.  The definition is in the header.  PyTorch is used only for device
memory and streams.
"""
from __future__ import annotations

import ctypes
from typing import Any, Dict, Optional, Tuple

import torch

from . import _lib
from ._handle import Handle, ptr

CLOUD_POINT_NAMES = _lib.CLOUD_POINT_NAMES
CLOUD_FRAME_NAMES = _lib.CLOUD_FRAME_NAMES


class CloudReadout(Handle):
    """A point-cloud read-out for h x w planes, at most `max_batch` frames and `max_points` written points per call.  stride (1..64) keeps
    every stride-th column and row; origin (x, y) is the pixel that becomes X = Y = 0, by default the crop centre ((w - 1) / 2, (h - 1) / 2).
    More points than max_points is not an error: the offsets are never capped, the frame rows count what was written, and `trim` reports
    `overflow`.  Creating it needs no device, `measure` does."""
    _destroy = "vistaf_cloud_destroy"

    def __init__(self, h: int, w: int, max_batch: int, max_points: int, stride: int = 1, origin: Optional[Tuple[float, float]] = None, device="cuda:0"):
        self.h, self.w, self.max_batch, self.max_points, self.stride = int(h), int(w), int(max_batch), int(max_points), int(stride)
        self.origin = ((self.w - 1) / 2.0, (self.h - 1) / 2.0) if origin is None else (float(origin[0]), float(origin[1]))
        self._open(device, need_device=False)
        self._call("vistaf_cloud_create", self.h, self.w, self.max_batch, self.max_points, self.stride, self.origin[0], self.origin[1],
                   ctypes.byref(self._h), on_device=False)

    def measure(self, depth, mm_per_px, depth_eps_mm: float, status=None, contact_index=None, out: Optional[Dict[str, torch.Tensor]] = None) -> Dict[str, torch.Tensor]:
        """depth [B,h,w] float32 (the height map of a predict), mm_per_px [B] float64, status [B] int32 or None (every frame OK; a frame whose
        status is not 0 has no points and a NaN row), contact_index [B,h,w] int8 or None (the index plane of the contacts table), device or
        host.  Returns device tensors: points [max_points,8] f32 (fields CLOUD_POINT_NAMES), pixel [max_points] i32 (y * w + x), label
        [max_points] i8 when a plane was given, offsets [B+1] i64 (the points of frame b are offsets[b] .. offsets[b+1]-1; never capped),
        frame [B,12] f64 (fields CLOUD_FRAME_NAMES, field 11 reserved).  Only the first min(offsets[B], max_points) entries of points, pixel
        and label are written; `trim` cuts them.  out: tensors "points", "pixel", "label" of the caller's own (contiguous, on the device,
        at least max_points long) to write into instead of new ones."""
        self._need_device("measure")
        dep = self._t(depth, torch.float32, (None, self.h, self.w), f"depth must be [B,{self.h},{self.w}]")
        b = int(dep.shape[0])
        msg = "mm_per_px and status must be [B] for the B frames of depth"
        mpp, sta = self._t(mm_per_px, torch.float64, (b,), msg), self._t(status, torch.int32, (b,), msg)
        idx = self._t(contact_index, torch.int8, dep.shape, "contact_index must have the shape of depth")
        if not 1 <= b <= self.max_batch:
            raise ValueError(f"batch {b} outside 1..max_batch {self.max_batch}")
        given = out or {}
        res: Dict[str, torch.Tensor] = {}
        for name, shape, dtype in (("points", (self.max_points, _lib.NCLOUD_POINT), torch.float32), ("pixel", (self.max_points,), torch.int32),
                                   ("label", (self.max_points,), torch.int8)):
            if name == "label" and idx is None:
                continue
            t = given.get(name)
            if t is None:
                t = torch.empty(shape, dtype=dtype, device=self.device)
            elif t.dtype != dtype or t.device != dep.device or not t.is_contiguous() or t.shape[0] < self.max_points or tuple(t.shape[1:]) != shape[1:]:
                raise ValueError(f"out[{name!r}] must be a contiguous {dtype} tensor [>={self.max_points}{', 8' if name == 'points' else ''}] on {self.device}")
            res[name] = t
        res["offsets"] = torch.empty((b + 1,), dtype=torch.int64, device=self.device)
        res["frame"] = torch.empty((b, _lib.NCLOUD_FRAME), dtype=torch.float64, device=self.device)
        self._call("vistaf_cloud_measure", self._h, dep.data_ptr(), mpp.data_ptr(), ptr(sta), ptr(idx), float(depth_eps_mm), b,
                   res["points"].data_ptr(), res["pixel"].data_ptr(), ptr(res.get("label")), res["offsets"].data_ptr(), res["frame"].data_ptr(),
                   self._stream())
        return res

    def trim(self, out: Dict[str, torch.Tensor]) -> Dict[str, Any]:
        """Synchronises once (reads offsets[B]) and returns views of the written part of points, pixel and label (when present), the
        offsets and frame rows as they are, `total` (the points of the batch) and `overflow` (total > max_points: the tail was dropped,
        which the frame rows' points_written tell per frame)."""
        total = int(out["offsets"][-1].item())
        n = min(total, self.max_points)
        res: Dict[str, Any] = {k: out[k][:n] for k in ("points", "pixel", "label") if k in out}
        res.update(offsets=out["offsets"], frame=out["frame"], total=total, overflow=total > self.max_points)
        return res
