"""Taxel read-out (include/vistaf_taxel.h): a depth plane reduced to a fixed array of cells and to the frame's wrench.

An extension with no counterpart in the reference.  The contacts table, the tracker and the shape read-out describe individual touches, rows
that move from frame to frame; a robot that wears the skin wants the same cells every frame -- a grid, rings and sectors of the ROI disc, or
patches of its own -- each with pixels, area, volume, mean and peak depth, centroid, a share of the frame's force and a pressure, plus the
frame's normal force, centre of pressure and tilting moments: [B, T, 12] and [B, 8] doubles instead of B depth maps.  `TaxelLayout` and the
builders are host code; `TaxelReadout.measure` runs on the device, from the height map, so no plane is copied to the host.  The definition
is in the header.  PyTorch is used only for device memory and streams.
"""
from __future__ import annotations

import ctypes
import math
from typing import Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib
from ._handle import Handle, ptr

TAXEL_NAMES = _lib.TAXEL_NAMES
TAXEL_FRAME_NAMES = _lib.TAXEL_FRAME_NAMES
NONE = _lib.TAXEL_NONE


class TaxelLayout:
    """The uint16 map [h, w] (taxel of every pixel, `NONE` = 0xFFFF for a pixel of no taxel), the number of taxels, the origin (x, y) in crop
    pixels the frame's moments are taken about, and optional names, one per taxel."""

    def __init__(self, taxel_map, n_taxels: int, origin: Tuple[float, float], names: Optional[Sequence[str]] = None):
        m = np.ascontiguousarray(taxel_map, dtype=np.uint16)
        if m.ndim != 2 or m.size == 0:
            raise ValueError("the taxel map must be [h, w]")
        self.map, self.n_taxels = m, int(n_taxels)
        self.origin = (float(origin[0]), float(origin[1]))
        if not 1 <= self.n_taxels <= 65535:
            raise ValueError("n_taxels must be 1..65535")
        if not (math.isfinite(self.origin[0]) and math.isfinite(self.origin[1])):
            raise ValueError("the origin must be finite")
        if ((m >= self.n_taxels) & (m != NONE)).any():
            raise ValueError("a map value is neither below n_taxels nor NONE (0xFFFF)")
        if names is not None and len(names) != self.n_taxels:
            raise ValueError("names must hold one name per taxel")
        self.names = list(names) if names is not None else None

    @property
    def shape(self) -> Tuple[int, int]:
        return int(self.map.shape[0]), int(self.map.shape[1])


def _inside(h: int, w: int, roi_circle) -> np.ndarray:
    cx, cy, r = roi_circle
    yy, xx = np.ogrid[:h, :w]
    return ((xx - cx) ** 2 + (yy - cy) ** 2) <= r * r           # the ROI disc as create_circular_mask draws it


def grid_layout(h: int, w: int, rows: int, cols: int, roi_circle=None) -> TaxelLayout:
    """rows x cols cells of as equal size as integer division allows: pixel (x, y) belongs to taxel (y*rows//h)*cols + x*cols//w, named
    "r<row>c<col>".  With roi_circle = (cx, cy, r) the pixels outside the disc belong to no taxel and the origin is the circle's centre,
    else the frame's centre ((w-1)/2, (h-1)/2)."""
    h, w, rows, cols = int(h), int(w), int(rows), int(cols)
    if not (1 <= rows <= h and 1 <= cols <= w) or rows * cols > 65535:
        raise ValueError("rows and cols must be 1..h and 1..w, at most 65535 cells")
    ry = (np.arange(h, dtype=np.int64) * rows) // h
    cx_ = (np.arange(w, dtype=np.int64) * cols) // w
    m = (ry[:, None] * cols + cx_[None, :]).astype(np.uint16)
    origin = ((w - 1) / 2.0, (h - 1) / 2.0)
    if roi_circle is not None:
        m[~_inside(h, w, roi_circle)] = NONE
        origin = (float(roi_circle[0]), float(roi_circle[1]))
    return TaxelLayout(m, rows * cols, origin, ["r%dc%d" % (r, c) for r in range(rows) for c in range(cols)])


def polar_layout(h: int, w: int, roi_circle, rings: int, sectors: int) -> TaxelLayout:
    """Rings of equal radial width and equal angular sectors about the centre of roi_circle = (cx, cy, r): a pixel at distance d <= r and
    angle a = atan2(y - cy, x - cx) mod 2 pi belongs to taxel min(floor(d*rings/r), rings-1)*sectors + min(floor(a*sectors/(2 pi)), sectors-1),
    named "ring<i>s<j>"; the pixels outside the disc belong to no taxel.  The origin is the centre."""
    h, w, rings, sectors = int(h), int(w), int(rings), int(sectors)
    cx, cy, r = (float(v) for v in roi_circle)
    if rings < 1 or sectors < 1 or rings * sectors > 65535 or not r > 0:
        raise ValueError("rings and sectors must be >= 1, at most 65535 cells, and the radius positive")
    yy, xx = np.mgrid[:h, :w]
    dx, dy = xx - cx, yy - cy
    ring = np.minimum(np.floor(np.sqrt(dx * dx + dy * dy) * rings / r), rings - 1).astype(np.int64)
    ang = np.mod(np.arctan2(dy, dx), 2.0 * np.pi)
    sec = np.minimum(np.floor(ang * sectors / (2.0 * np.pi)), sectors - 1).astype(np.int64)
    m = (ring * sectors + sec).astype(np.uint16)
    m[~_inside(h, w, (cx, cy, r))] = NONE
    return TaxelLayout(m, rings * sectors, (cx, cy), ["ring%ds%d" % (i, j) for i in range(rings) for j in range(sectors)])


def from_map(array, origin=None, n_taxels: Optional[int] = None, names=None) -> TaxelLayout:
    """Any integer map [h, w]: values 0..n_taxels-1, a negative value or 0xFFFF for no taxel.  n_taxels defaults to the largest id + 1,
    the origin to the frame's centre."""
    a = np.asarray(array)
    if a.ndim != 2 or a.size == 0 or not np.issubdtype(a.dtype, np.integer):
        raise ValueError("the taxel map must be an integer array [h, w]")
    a = a.astype(np.int64)
    none = (a < 0) | (a == NONE)
    if (a > NONE).any():
        raise ValueError("taxel ids must be below 65535")
    if n_taxels is None:
        n_taxels = int(a[~none].max()) + 1 if (~none).any() else 1
    h, w = a.shape
    return TaxelLayout(np.where(none, NONE, a).astype(np.uint16), n_taxels, origin if origin is not None else ((w - 1) / 2.0, (h - 1) / 2.0), names)


class TaxelReadout(Handle):
    """A taxel read-out for planes of the layout's size, at most `max_batch` frames per call.  The layout is inverted here, on the host;
    `layout_info` needs no device, `measure` does."""
    _destroy = "vistaf_taxel_destroy"

    def __init__(self, layout: TaxelLayout, max_batch: int, device="cuda:0"):
        self.layout, self.max_batch = layout, int(max_batch)
        self.h, self.w = layout.shape
        self.n_taxels = layout.n_taxels
        self._open(device, need_device=False)
        self._call("vistaf_taxel_create", self.h, self.w, self.max_batch, layout.map.ctypes.data, self.n_taxels, layout.origin[0], layout.origin[1],
                   ctypes.byref(self._h), on_device=False)

    def layout_info(self) -> np.ndarray:
        """[T, 4] float64: pixels of the taxel, mean x and mean y of its pixels (NaN for a taxel without pixels), reserved."""
        info = np.empty((self.n_taxels, 4), dtype=np.float64)
        self._call("vistaf_taxel_layout_info", self._h, info.ctypes.data, on_device=False)
        return info

    def measure(self, depth_mm, mm_per_px, depth_eps_mm: float, force_N=None, status=None):
        """depth_mm [B,h,w] float32 (the height map of a predict), mm_per_px [B] float64, force_N [B] float64 or None (forces, pressures and
        moments are then NaN), status [B] int32 or None (every frame OK; a frame whose status is not 0 gets NaN rows), device or host.
        Returns the device tensors {"taxels": [B,T,12] f64 (fields TAXEL_NAMES), "frame": [B,8] f64 (fields TAXEL_FRAME_NAMES)}."""
        self._need_device("measure")
        dep = self._t(depth_mm, torch.float32, (None, self.h, self.w), f"depth_mm must be [B,{self.h},{self.w}]")
        b = int(dep.shape[0])
        msg = "mm_per_px, force_N and status must be [B] for the B frames of depth_mm"
        mpp, frc, sta = self._t(mm_per_px, torch.float64, (b,), msg), self._t(force_N, torch.float64, (b,), msg), self._t(status, torch.int32, (b,), msg)
        if not 1 <= b <= self.max_batch:
            raise ValueError(f"batch {b} outside 1..max_batch {self.max_batch}")
        if not math.isfinite(float(depth_eps_mm)):
            raise ValueError("depth_eps_mm must be finite")
        out = {"taxels": torch.empty((b, self.n_taxels, _lib.NTAXEL), dtype=torch.float64, device=self.device),
               "frame": torch.empty((b, _lib.NTAXELFRAME), dtype=torch.float64, device=self.device)}
        self._call("vistaf_taxel_measure", self._h, dep.data_ptr(), mpp.data_ptr(), ptr(frc), ptr(sta), float(depth_eps_mm), b,
                   out["taxels"].data_ptr(), out["frame"].data_ptr(), self._stream())
        return out
