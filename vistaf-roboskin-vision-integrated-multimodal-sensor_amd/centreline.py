"""Centreline read-out (include_ext/vistaf_centreline.h): skeleton, axis path, length, width profile, end tangents and bend of every contact.

An extension with no counterpart in the reference.  The other per-contact read-outs describe a touch as a body, a boundary, a surface and a
known part; `contact_centrelines` describes an elongated one -- a cable, a rod, the edge of a plate -- by the line it runs along: what
`cv2.ximgproc.thinning`, `distanceTransform` and a graph walk would give on the index plane, on the device, so the plane is not copied to the
host to follow a cable.  Two plain functions of the library and no handle: the workspace is a tensor of the caller's.  The definition is in
the header.  PyTorch is used only for device memory and streams.
"""
from __future__ import annotations

from typing import Any, Dict, Optional

import torch

from . import _lib
from ._handle import call, stream
from ._workspace import Workspace, table_inputs
from ._workspace import workspace_bytes as _workspace_bytes

CENTRELINE_NAMES = _lib.CENTRELINE_NAMES
CENTRELINE_STATUS = _lib.CENTRELINE_STATUS


def workspace_bytes(h: int, w: int, batch: int, max_contacts: int) -> int:
    """the bytes of the workspace `contact_centrelines` needs for `batch` frames of h x w and tables of max_contacts rows; ValueError for
    sizes the read-out does not take.  Needs no device."""
    return _workspace_bytes(CentrelineWorkspace._sizer, h, w, batch, max_contacts)


def default_max_stations(h: int, w: int) -> int:
    """the station capacity per frame used when none is given: 2 * (h + w), a path along the whole border of the frame"""
    return 2 * (int(h) + int(w))


class CentrelineWorkspace(Workspace):
    """The device memory of the read-out for up to `batch` frames of h x w and tables of max_contacts rows: one tensor, nothing of the
    library's.  `close()` drops it."""

    _sizer = "vistaf_centreline_workspace_bytes"

    def __init__(self, h: int, w: int, batch: int, max_contacts: int = 8, device="cuda:0"):
        super().__init__(device, h, w, batch, max_contacts)


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
    dev, idx, tab, cnt, mpp, dep, b, h, w, k = table_inputs("contact_centrelines", contact_index, contacts, count, mm_per_px, device, depth_mm,
                                                            "depth_mm must be [B,h,w] like contact_index")
    v = default_max_stations(h, w) if max_stations is None else int(max_stations)
    if v < 0:
        raise ValueError("max_stations must be >= 0")
    if not 1 <= int(tangent_span) <= 1024:
        raise ValueError("tangent_span must be 1..1024")
    ws = CentrelineWorkspace.fitting(workspace, dev, h, w, b, k)
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
