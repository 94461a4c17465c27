"""Contact outline read-out (include_ext/vistaf_outline.h): boundary loops, holes, corner polyline, convex hull and caliper box of every contact.

An extension with no counterpart in the reference.  `FtpSensor.contacts(K, index_plane=True)` says where a touch is and `ContactShapes` gives
the ellipse of its footprint; `contact_outlines` gives the footprint's outline -- what `cv2.findContours`, `convexHull` and `minAreaRect`
would give on the index plane -- on the device, from the index plane and the table, so the plane is not copied to the host to tell a ring from
a bar.  Two plain functions of the library and no handle: the workspace is a tensor of the caller's.  The definition is in the header.
PyTorch is used only for device memory and streams.
"""
from __future__ import annotations

from typing import Any, Dict, Optional

import torch

from . import _lib
from ._handle import call, stream
from ._workspace import Workspace, table_inputs
from ._workspace import workspace_bytes as _workspace_bytes

OUTLINE_NAMES = _lib.OUTLINE_NAMES


def workspace_bytes(h: int, w: int, batch: int, max_contacts: int) -> int:
    """the bytes of the workspace `contact_outlines` needs for `batch` frames of h x w and tables of max_contacts rows; ValueError for sizes
    the read-out does not take.  Needs no device."""
    return _workspace_bytes(OutlineWorkspace._sizer, h, w, batch, max_contacts)


def default_max_vertices(h: int, w: int) -> int:
    """the polyline capacity per frame used when none is given: 4 * (h + w) vertices, the corners of a staircase around the whole frame twice over"""
    return 4 * (int(h) + int(w))


class OutlineWorkspace(Workspace):
    """The device memory of the read-out for up to `batch` frames of h x w and tables of max_contacts rows: one tensor, nothing of the
    library's.  `close()` drops it."""

    _sizer = "vistaf_outline_workspace_bytes"

    def __init__(self, h: int, w: int, batch: int, max_contacts: int = 8, device="cuda:0"):
        super().__init__(device, h, w, batch, max_contacts)


def contact_outlines(contact_index, contacts, count, mm_per_px, max_vertices: Optional[int] = None, workspace: Optional[OutlineWorkspace] = None,
                     device="cuda:0") -> Dict[str, torch.Tensor]:
    """contact_index [B,h,w] int8, contacts [B,K,16] float64 and count [B] int32 as `FtpSensor.contacts(K, index_plane=True)` returns them,
    mm_per_px [B] float64 (device or host).  Returns device tensors: outlines [B,K,24] f64 (fields OUTLINE_NAMES, unused rows and fields
    NaN), vertices [B,V,2] i32 ((x, y) lattice corners of the principal loops) and offsets [B,K+1] i32 (row k of frame b is
    vertices[b, offsets[b,k]:offsets[b,k+1]]); only `outlines` with max_vertices=0.  V = max_vertices per frame, by default
    `default_max_vertices(h, w)` = 4 * (h + w); a row that does not fit, and every row after it, is left out and shows
    corners_written < corners (`trim` reports it).  workspace: an OutlineWorkspace that fits, else one is made for the call."""
    dev, idx, tab, cnt, mpp, _, b, h, w, k = table_inputs("contact_outlines", contact_index, contacts, count, mm_per_px, device)
    v = default_max_vertices(h, w) if max_vertices is None else int(max_vertices)
    if v < 0:
        raise ValueError("max_vertices must be >= 0")
    ws = OutlineWorkspace.fitting(workspace, dev, h, w, b, k)
    res = {"outlines": torch.empty((b, k, _lib.NOUTLINE), dtype=torch.float64, device=dev)}
    if v > 0:
        res["vertices"] = torch.empty((b, v, 2), dtype=torch.int32, device=dev)
        res["offsets"] = torch.empty((b, k + 1), dtype=torch.int32, device=dev)
    call(dev, "vistaf_outline_measure", idx.data_ptr(), tab.data_ptr(), cnt.data_ptr(), mpp.data_ptr(), b, h, w, k, v, res["outlines"].data_ptr(),
         res["vertices"].data_ptr() if v else None, res["offsets"].data_ptr() if v else None, ws.pointer(), ws.nbytes, stream(dev))
    return res


def trim(result: Dict[str, torch.Tensor]) -> Dict[str, Any]:
    """Synchronises once and returns {"polylines": per frame the list of [n,2] int32 arrays of the rows that were written (a row in use
    without a pixel gives an empty array), "overflow": whether any row's corners were left out}."""
    out = result["outlines"].cpu().numpy()
    corners, written = out[..., OUTLINE_NAMES.index("corners")], out[..., OUTLINE_NAMES.index("corners_written")]
    used = corners == corners
    res: Dict[str, Any] = {"polylines": [], "overflow": bool((written[used] < corners[used]).any())}
    if "vertices" not in result:
        res["polylines"] = [[] for _ in range(out.shape[0])]
        return res
    verts, offs = result["vertices"].cpu().numpy(), result["offsets"].cpu().numpy()
    for b in range(out.shape[0]):
        res["polylines"].append([verts[b, offs[b, k]:offs[b, k + 1]].copy() for k in range(out.shape[1]) if used[b, k] and written[b, k] == corners[b, k]])
    return res
