"""Centreline read-out (include_ext/vistaf_centreline.h): skeleton, axis path, length, width profile, end tangents and bend of every contact.

An extension with no counterpart in the reference.  The other per-contact read-outs describe a touch as a body, a boundary, a surface and a
known part; `contact_centrelines` describes an elongated one -- a cable, a rod, the edge of a plate -- by the line it runs along: what
`cv2.ximgproc.thinning`, `distanceTransform` and a graph walk would give on the index plane, on the device, so the plane is not copied to the
host to follow a cable.  Two plain functions of the library and no handle: the workspace is a tensor of the caller's.  The definition is in
the header.  PyTorch is used only for device memory and streams.
"""
from __future__ import annotations

import ctypes
from typing import Any, Dict, Optional

import torch

from . import _lib
from ._handle import call, stream

CENTRELINE_NAMES = _lib.CENTRELINE_NAMES
CENTRELINE_STATUS = _lib.CENTRELINE_STATUS


def workspace_bytes(h: int, w: int, batch: int, max_contacts: int) -> int:
    """the bytes of the workspace `contact_centrelines` needs for `batch` frames of h x w and tables of max_contacts rows; ValueError for
    sizes the read-out does not take.  Needs no device."""
    n = ctypes.c_size_t()
    call(None, "vistaf_centreline_workspace_bytes", int(h), int(w), int(batch), int(max_contacts), ctypes.byref(n))
    return int(n.value)


def default_max_stations(h: int, w: int) -> int:
    """the station capacity per frame used when none is given: 2 * (h + w), a path along the whole border of the frame"""
    return 2 * (int(h) + int(w))


class CentrelineWorkspace:
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


def contact_centrelines(contact_index, contacts, count, mm_per_px, depth_mm=None, tangent_span: int = 8, max_stations: Optional[int] = None,
                        skeleton: bool = True, workspace: Optional[CentrelineWorkspace] = None, device="cuda:0") -> Dict[str, torch.Tensor]:
    """contact_index [B,h,w] int8, contacts [B,K,16] float64 and count [B] int32 as `FtpSensor.contacts(K, index_plane=True)` returns them,
    mm_per_px [B] float64 (device or host), depth_mm [B,h,w] float32 or None (then the depth fields are NaN).  Returns device tensors:
    centrelines [B,K,40] f64 (fields CENTRELINE_NAMES, unused rows and fields NaN), stations [B,V,2] i32 (the (x, y) of the axis path from
    end A to end B), station_d2 [B,V] i32 (their exact squared distance to the rim: the width profile) and offsets [B,K+1] i32 (row k of
    frame b is stations[b, offsets[b,k]:offsets[b,k+1]]); without the three with max_stations=0; skeleton [B,h,w] i8 (k on the skeleton of
    row k, -1 elsewhere) unless skeleton=False.  V = max_stations per frame, by default `default_max_stations(h, w)` = 2 * (h + w); a row
    that does not fit, and every row after it, is left out and shows stations_written < stations and the `truncated` status flag (`trim`
    reports it).  tangent_span: the stations an end tangent and an end depth reach over, 1..1024.  workspace: a CentrelineWorkspace that
    fits, else one is made for the call."""
    if not torch.cuda.is_available():
        raise RuntimeError("contact_centrelines needs a HIP device (torch.cuda.is_available() is False); there is no CPU path")
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
    dep = None
    if depth_mm is not None:
        dep = torch.as_tensor(depth_mm).to(dev, torch.float32).contiguous()
        if tuple(dep.shape) != (b, h, w):
            raise ValueError("depth_mm must be [B,h,w] like contact_index")
    v = default_max_stations(h, w) if max_stations is None else int(max_stations)
    if v < 0:
        raise ValueError("max_stations must be >= 0")
    if not 1 <= int(tangent_span) <= 1024:
        raise ValueError("tangent_span must be 1..1024")
    ws = workspace if workspace is not None and workspace.fits(h, w, b, k) and workspace.device == dev else CentrelineWorkspace(h, w, b, k, dev)
    res = {"centrelines": torch.empty((b, k, _lib.NCENTRELINE), dtype=torch.float64, device=dev)}
    if v > 0:
        res["stations"] = torch.empty((b, v, 2), dtype=torch.int32, device=dev)
        res["station_d2"] = torch.empty((b, v), dtype=torch.int32, device=dev)
        res["offsets"] = torch.empty((b, k + 1), dtype=torch.int32, device=dev)
    if skeleton:
        res["skeleton"] = torch.empty((b, h, w), dtype=torch.int8, device=dev)
    call(dev, "vistaf_centreline_measure", idx.data_ptr(), tab.data_ptr(), cnt.data_ptr(), mpp.data_ptr(), dep.data_ptr() if dep is not None else None,
         b, h, w, k, int(tangent_span), v, res["centrelines"].data_ptr(), res["stations"].data_ptr() if v else None,
         res["station_d2"].data_ptr() if v else None, res["offsets"].data_ptr() if v else None, res["skeleton"].data_ptr() if skeleton else None,
         ws.pointer(), ws.nbytes, stream(dev))
    return res


def trim(result: Dict[str, torch.Tensor]) -> Dict[str, Any]:
    """Synchronises once and returns {"stations": per frame the list of [n,2] int32 arrays of the rows that were written (a row in use
    without a pixel gives an empty array), "d2": the [n] int32 arrays that go with them, "overflow": whether any row's stations were left
    out}."""
    out = result["centrelines"].cpu().numpy()
    stations, written = out[..., CENTRELINE_NAMES.index("stations")], out[..., CENTRELINE_NAMES.index("stations_written")]
    used = stations == stations
    res: Dict[str, Any] = {"stations": [], "d2": [], "overflow": bool((written[used] < stations[used]).any())}
    if "stations" not in result:
        res["stations"] = [[] for _ in range(out.shape[0])]
        res["d2"] = [[] for _ in range(out.shape[0])]
        return res
    st, d2, offs = result["stations"].cpu().numpy(), result["station_d2"].cpu().numpy(), result["offsets"].cpu().numpy()
    for b in range(out.shape[0]):
        rows = [k for k in range(out.shape[1]) if used[b, k] and written[b, k] == stations[b, k]]
        res["stations"].append([st[b, offs[b, k]:offs[b, k + 1]].copy() for k in rows])
        res["d2"].append([d2[b, offs[b, k]:offs[b, k + 1]].copy() for k in rows])
    return res
