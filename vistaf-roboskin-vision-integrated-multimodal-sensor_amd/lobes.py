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

from typing import Any, Dict, Optional

import torch

from . import _lib
from ._handle import call, stream
from ._workspace import Workspace, table_inputs
from ._workspace import workspace_bytes as _workspace_bytes

LOBE_NAMES = _lib.LOBE_NAMES
LOBE_ROW_NAMES = _lib.LOBE_ROW_NAMES
LOBE_STATUS = _lib.LOBE_STATUS
DEFAULT_MIN_PROMINENCE_MM, DEFAULT_MIN_PROMINENCE_FRAC = 0.02, 0.10


def workspace_bytes(h: int, w: int, batch: int, max_contacts: int) -> int:
    """the bytes of the workspace `contact_lobes` needs for `batch` frames of h x w and tables of max_contacts rows; ValueError for sizes the
    read-out does not take.  Needs no device."""
    return _workspace_bytes(LobesWorkspace._sizer, h, w, batch, max_contacts)


class LobesWorkspace(Workspace):
    """The device memory of the read-out for up to `batch` frames of h x w and tables of max_contacts rows: one tensor, nothing of the
    library's.  `close()` drops it."""

    _sizer = "vistaf_lobes_workspace_bytes"

    def __init__(self, h: int, w: int, batch: int, max_contacts: int = 8, device="cuda:0"):
        super().__init__(device, h, w, batch, max_contacts)


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
    dev, idx, tab, cnt, mpp, dep, b, h, w, k = table_inputs("contact_lobes", contact_index, contacts, count, mm_per_px, device, depth_mm,
                                                            "depth_mm must be [B,h,w] like contact_index")
    if dep is None:
        raise ValueError("depth_mm is required: the lobes are those of the depth relief")
    n = int(max_lobes)
    if not 1 <= n <= _lib.LOBES_MAX:
        raise ValueError(f"max_lobes must be 1..{_lib.LOBES_MAX}")
    ws = LobesWorkspace.fitting(workspace, dev, h, w, b, k)
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
