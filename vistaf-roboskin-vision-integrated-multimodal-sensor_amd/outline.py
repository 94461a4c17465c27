"""Contact outline read-out (include_ext/vistaf_outline.h): boundary loops, holes, corner polyline, convex hull and caliper box of every contact.

An extension with no counterpart in the reference.  `FtpSensor.contacts(K, index_plane=True)` says where a touch is and `ContactShapes` gives
the ellipse of its footprint; `contact_outlines` gives the footprint's outline -- what `cv2.findContours`, `convexHull` and `minAreaRect`
would give on the index plane -- on the device, from the index plane and the table, so the plane is not copied to the host to tell a ring from
a bar.  Two plain functions of the library and no handle: the workspace is a tensor of the caller's.  The definition is in the header.
PyTorch is used only for device memory and streams.
"""
from __future__ import annotations

import ctypes
from typing import Any, Dict, Optional

import torch

from . import _lib
from ._handle import call, stream

OUTLINE_NAMES = _lib.OUTLINE_NAMES


def workspace_bytes(h: int, w: int, batch: int, max_contacts: int) -> int:
    """the bytes of the workspace `contact_outlines` needs for `batch` frames of h x w and tables of max_contacts rows; ValueError for sizes
    the read-out does not take.  Needs no device."""
    n = ctypes.c_size_t()
    call(None, "vistaf_outline_workspace_bytes", int(h), int(w), int(batch), int(max_contacts), ctypes.byref(n))
    return int(n.value)


def default_max_vertices(h: int, w: int) -> int:
    """the polyline capacity per frame used when none is given: 4 * (h + w) vertices, the corners of a staircase around the whole frame twice over"""
    return 4 * (int(h) + int(w))


class OutlineWorkspace:
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


def contact_outlines(contact_index, contacts, count, mm_per_px, max_vertices: Optional[int] = None, workspace: Optional[OutlineWorkspace] = None,
                     device="cuda:0") -> Dict[str, torch.Tensor]:
    """contact_index [B,h,w] int8, contacts [B,K,16] float64 and count [B] int32 as `FtpSensor.contacts(K, index_plane=True)` returns them,
    mm_per_px [B] float64 (device or host).  Returns device tensors: outlines [B,K,24] f64 (fields OUTLINE_NAMES, unused rows and fields
    NaN), vertices [B,V,2] i32 ((x, y) lattice corners of the principal loops) and offsets [B,K+1] i32 (row k of frame b is
    vertices[b, offsets[b,k]:offsets[b,k+1]]); only `outlines` with max_vertices=0.  V = max_vertices per frame, by default
    `default_max_vertices(h, w)` = 4 * (h + w); a row that does not fit, and every row after it, is left out and shows
    corners_written < corners (`trim` reports it).  workspace: an OutlineWorkspace that fits, else one is made for the call."""
    if not torch.cuda.is_available():
        raise RuntimeError("contact_outlines needs a HIP device (torch.cuda.is_available() is False); there is no CPU path")
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
    v = default_max_vertices(h, w) if max_vertices is None else int(max_vertices)
    if v < 0:
        raise ValueError("max_vertices must be >= 0")
    ws = workspace if workspace is not None and workspace.fits(h, w, b, k) and workspace.device == dev else OutlineWorkspace(h, w, b, k, dev)
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
