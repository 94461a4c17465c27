"""Lobe read-out (include_ext/vistaf_lobes.h): the depth maxima inside every contact, their prominence, the lobes a merged contact splits into
and the table of those lobes in the layout of the contacts table.

An extension with no counterpart in the reference.  Every other per-contact read-out is keyed on one row of the contacts table, one connected
footprint; two fingertips pressed a few millimetres apart on a soft skin leave ONE footprint with two depth maxima.  `contact_lobes` says how
many touches one contact holds and hands back `split_contacts`, `split_count`, `split_index`: a table `ContactTracker.update`,
`ContactShapes.measure`, `contact_centrelines` and the other read-outs take unchanged.  Two plain functions of the library and no handle: the
workspace is a tensor of the caller's.  The definition is in the header.  PyTorch is used only for device memory and streams.

The defaults of the two prominences (a maximum must stand DEFAULT_MIN_PROMINENCE_MM = 0.02 mm and DEFAULT_MIN_PROMINENCE_FRAC = 0.10 of the
contact's greatest depth above its saddle to be a touch of its own) are a judgement about the noise of a smoothed depth map that nobody has
measured on this sensor; `min_prominence_frac` exists so that one setting serves light and heavy touches.
"""
from __future__ import annotations

import ctypes
from typing import Any, Dict, Optional

import torch

from . import _lib
from ._handle import call, stream

LOBE_NAMES = _lib.LOBE_NAMES
LOBE_ROW_NAMES = _lib.LOBE_ROW_NAMES
LOBE_STATUS = _lib.LOBE_STATUS
DEFAULT_MIN_PROMINENCE_MM, DEFAULT_MIN_PROMINENCE_FRAC = 0.02, 0.10


def workspace_bytes(h: int, w: int, batch: int, max_contacts: int) -> int:
    """the bytes of the workspace `contact_lobes` needs for `batch` frames of h x w and tables of max_contacts rows; ValueError for sizes the
    read-out does not take.  Needs no device."""
    n = ctypes.c_size_t()
    call(None, "vistaf_lobes_workspace_bytes", int(h), int(w), int(batch), int(max_contacts), ctypes.byref(n))
    return int(n.value)


class LobesWorkspace:
    """The device memory of the read-out for up to `batch` frames of h x w and tables of max_contacts rows: one tensor, nothing of the
    library's.  `close()` drops it."""

    def __init__(self, h: int, w: int, batch: int, max_contacts: int = 8, device="cuda:0"):
        self.h, self.w, self.batch, self.max_contacts = int(h), int(w), int(batch), int(max_contacts)
        self.device = torch.device(device)
        self.nbytes = workspace_bytes(self.h, self.w, self.batch, self.max_contacts)
        self.buffer: Optional[torch.Tensor] = torch.empty((self.nbytes + 255,), dtype=torch.uint8, device=self.device)

    def fits(self, h: int, w: int, batch: int, max_contacts: int) -> bool:
        return self.buffer is not None and (self.h, self.w, self.max_contacts) == (int(h), int(w), int(max_contacts)) and int(batch) <= self.batch

    def pointer(self) -> int:
        """the first 256-byte aligned address of the buffer"""
        return (self.buffer.data_ptr() + 255) & ~255

    def close(self):
        self.buffer = None


def contact_lobes(contact_index, contacts, count, mm_per_px, depth_mm, max_lobes: int = 4, min_prominence_mm: float = DEFAULT_MIN_PROMINENCE_MM,
                  min_prominence_frac: float = DEFAULT_MIN_PROMINENCE_FRAC, depth_eps_mm: float = 0.0, split: bool = True, lobe_index: bool = True,
                  workspace: Optional[LobesWorkspace] = None, device="cuda:0") -> Dict[str, torch.Tensor]:
    """contact_index [B,h,w] int8, contacts [B,K,16] float64 and count [B] int32 as `FtpSensor.contacts(K, index_plane=True)` returns them,
    mm_per_px [B] float64 (device or host), depth_mm [B,h,w] float32.  Returns device tensors: lobes [B,K,max_lobes,16] f64 (fields
    LOBE_NAMES, records behind peaks_written NaN), lobe_rows [B,K,12] f64 (fields LOBE_ROW_NAMES), lobe_index [B,h,w] i8 (the lobe number of
    every pixel of a row in use, -2 on lobes beyond max_lobes, -1 elsewhere) unless lobe_index=False, and with split=True split_contacts
    [B,K,16] f64, split_count [B] i32, split_index [B,h,w] i8 -- the written lobes as a contacts table, its `force_N` holding each lobe's
    SHARE of its parent's force -- and split_parent [B,K,2] i32, the (row, lobe) every split row came from.  max_lobes 1..64; a maximum is
    a touch of its own when its prominence exceeds max(min_prominence_mm, min_prominence_frac * the contact's greatest depth) (the module
    docstring on the defaults); depth_eps_mm: the session's, for contact_pixels and the sums.  workspace: a LobesWorkspace that fits, else
    one is made for the call."""
    if not torch.cuda.is_available():
        raise RuntimeError("contact_lobes needs a HIP device (torch.cuda.is_available() is False); there is no CPU path")
    idx = torch.as_tensor(contact_index)
    dev = idx.device if idx.is_cuda else torch.device(device)
    idx = idx.to(dev, torch.int8).contiguous()
    if idx.dim() != 3:
        raise ValueError("contact_index must be [B,h,w]")
    b, h, w = (int(v) for v in idx.shape)
    tab = torch.as_tensor(contacts).to(dev, torch.float64).contiguous()
    if tab.dim() != 3 or tab.shape[0] != b or tab.shape[2] != _lib.NCONTACT or not 1 <= tab.shape[1] <= _lib.MAX_CONTACTS:
        raise ValueError(f"contacts must be [B,K,{_lib.NCONTACT}] with K in 1..{_lib.MAX_CONTACTS} for the B frames of contact_index")
    k = int(tab.shape[1])
    cnt, mpp = torch.as_tensor(count).to(dev, torch.int32).contiguous(), torch.as_tensor(mm_per_px).to(dev, torch.float64).contiguous()
    if tuple(cnt.shape) != (b,) or tuple(mpp.shape) != (b,):
        raise ValueError("count and mm_per_px must be [B] for the B frames of contact_index")
    if depth_mm is None:
        raise ValueError("depth_mm is required: the lobes are those of the depth relief")
    dep = torch.as_tensor(depth_mm).to(dev, torch.float32).contiguous()
    if tuple(dep.shape) != (b, h, w):
        raise ValueError("depth_mm must be [B,h,w] like contact_index")
    n = int(max_lobes)
    if not 1 <= n <= _lib.LOBES_MAX:
        raise ValueError(f"max_lobes must be 1..{_lib.LOBES_MAX}")
    ws = workspace if workspace is not None and workspace.fits(h, w, b, k) and workspace.device == dev else LobesWorkspace(h, w, b, k, dev)
    res = {"lobes": torch.empty((b, k, n, _lib.NLOBE), dtype=torch.float64, device=dev),
           "lobe_rows": torch.empty((b, k, _lib.NLOBEROW), dtype=torch.float64, device=dev)}
    if lobe_index:
        res["lobe_index"] = torch.empty((b, h, w), dtype=torch.int8, device=dev)
    if split:
        res["split_contacts"] = torch.empty((b, k, _lib.NCONTACT), dtype=torch.float64, device=dev)
        res["split_count"] = torch.empty((b,), dtype=torch.int32, device=dev)
        res["split_index"] = torch.empty((b, h, w), dtype=torch.int8, device=dev)
        res["split_parent"] = torch.empty((b, k, 2), dtype=torch.int32, device=dev)

    def ptr(name):
        return res[name].data_ptr() if name in res else None
    call(dev, "vistaf_lobes_measure", idx.data_ptr(), tab.data_ptr(), cnt.data_ptr(), mpp.data_ptr(), dep.data_ptr(), b, h, w, k, n,
         float(min_prominence_mm), float(min_prominence_frac), float(depth_eps_mm), res["lobes"].data_ptr(), res["lobe_rows"].data_ptr(), ptr("lobe_index"),
         ptr("split_contacts"), ptr("split_count"), ptr("split_index"), ptr("split_parent"), ws.pointer(), ws.nbytes, stream(dev))
    return res


def trim(result: Dict[str, torch.Tensor]) -> Dict[str, Any]:
    """Synchronises once and returns {"lobes": per frame, per row in use, the [peaks_written,16] float64 array of its lobe records (a row
    without a pixel gives an empty array), "overflow": whether any row has more peaks than were written}."""
    rows, lobes = result["lobe_rows"].cpu().numpy(), result["lobes"].cpu().numpy()
    peaks, written = rows[..., LOBE_ROW_NAMES.index("peaks")], rows[..., LOBE_ROW_NAMES.index("peaks_written")]
    used = peaks == peaks
    res: Dict[str, Any] = {"lobes": [], "overflow": bool((written[used] < peaks[used]).any())}
    for b in range(rows.shape[0]):
        res["lobes"].append([lobes[b, k, :int(written[b, k])].copy() for k in range(rows.shape[1]) if used[b, k]])
    return res
