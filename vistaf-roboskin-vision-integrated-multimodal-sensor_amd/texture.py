"""Surface texture read-out (include_ext/vistaf_texture.h): roughness, lay and pitch of every contact.

An extension with no counterpart in the reference.  `ContactShapes` fits the cap of a touch and keeps the rms of what is left;
`contact_textures` keeps the rest: the form-removed depth of every contact, its ISO 25178-2 height and slope parameters, the direction of its
dominant gradient (the lay is perpendicular to it), its normalised autocorrelation over a window of lags, the fastest-decay length and texture
aspect ratio of the central lobe and the pitch of a periodic surface -- on the device, so the depth plane is not copied to the host to tell a
thread from a rod.  Two plain functions of the library and no handle: the workspace is a tensor of the caller's.  The definition is in the
header.  PyTorch is used only for device memory and streams.
"""
from __future__ import annotations

from typing import Dict, Optional

import torch

from . import _lib
from ._handle import call, stream
from ._workspace import Workspace, table_inputs
from ._workspace import workspace_bytes as _workspace_bytes

TEXTURE_NAMES = _lib.TEXTURE_NAMES
TEXTURE_FORM = _lib.TEXTURE_FORM


def workspace_bytes(h: int, w: int, max_batch: int, max_contacts: int, max_lag: int) -> int:
    """the bytes of the workspace `contact_textures` needs for up to max_batch frames of h x w, tables of max_contacts rows and windows of
    max_lag; ValueError for sizes the read-out does not take.  Needs no device."""
    return _workspace_bytes(TextureWorkspace._sizer, h, w, max_batch, max_contacts, max_lag)


class TextureWorkspace(Workspace):
    """The device memory of the read-out for up to `batch` frames of h x w, tables of max_contacts rows and windows of max_lag: one tensor,
    nothing of the library's.  `close()` drops it."""

    _sizer = "vistaf_texture_workspace_bytes"
    max_lag = property(lambda self: self.key[3])

    def __init__(self, h: int, w: int, batch: int, max_contacts: int = 8, max_lag: int = 8, device="cuda:0"):
        super().__init__(device, h, w, batch, max_contacts, max_lag)


def contact_textures(depth, contact_index, contacts, count, mm_per_px, eps: float, ws: Optional[TextureWorkspace] = None,
                     eval_min_fraction: float = 0.5, form_degree: int = 2, max_lag: int = 8, acf_threshold: float = 0.2, peak_min: float = 0.3,
                     device="cuda:0") -> Dict[str, torch.Tensor]:
    """depth [B,h,w] float32 (the height map of a predict), contact_index [B,h,w] int8, contacts [B,K,16] float64 and count [B] int32 as
    `FtpSensor.contacts(K, index_plane=True)` returns them, mm_per_px [B] float64 (device or host), eps the session's depth_eps_mm.
    eval_min_fraction: a pixel is evaluated when its depth is at least this share of the contact's peak (the fit pixels of the shape read-out);
    form_degree 0, 1 or 2: the polynomial taken away; max_lag L in 2..31: the autocorrelation window is (2L+1) x (2L+1); acf_threshold: the
    level that bounds the central lobe; peak_min: the least autocorrelation of a pitch peak.  Returns device tensors: textures [B,K,40] f64
    (fields TEXTURE_NAMES, unused rows and fields NaN), residual [B,h,w] f32 (NaN where no residual is defined) and acf [B,K,2L+1,2L+1] f64
    (entry [dy+L][dx+L], NaN for an invalid lag).  ws: a TextureWorkspace that fits, else one is made for the call."""
    dev, idx, tab, cnt, mpp, dep, b, h, w, k = table_inputs("contact_textures", contact_index, contacts, count, mm_per_px, device, depth,
                                                            "depth must be [B,h,w] as contact_index")
    lag = int(max_lag)
    if not _lib.TEXTURE_MIN_LAG <= lag <= _lib.TEXTURE_MAX_LAG:
        raise ValueError(f"max_lag must be {_lib.TEXTURE_MIN_LAG}..{_lib.TEXTURE_MAX_LAG}")
    work = TextureWorkspace.fitting(ws, dev, h, w, b, k, lag)
    d = 2 * lag + 1
    res = {"textures": torch.empty((b, k, _lib.NTEXTURE), dtype=torch.float64, device=dev),
           "residual": torch.empty((b, h, w), dtype=torch.float32, device=dev),
           "acf": torch.empty((b, k, d, d), dtype=torch.float64, device=dev)}
    call(dev, "vistaf_texture_measure", dep.data_ptr(), idx.data_ptr(), tab.data_ptr(), cnt.data_ptr(), mpp.data_ptr(), float(eps),
         float(eval_min_fraction), int(form_degree), lag, float(acf_threshold), float(peak_min), h, w, b, k, res["textures"].data_ptr(),
         res["residual"].data_ptr(), res["acf"].data_ptr(), work.pointer(), work.nbytes, stream(dev))
    return res
