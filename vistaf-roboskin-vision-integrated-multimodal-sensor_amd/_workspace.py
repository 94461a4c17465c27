"""What the read-outs with two plain functions of the library and a workspace of the caller's share -- outline, texture, match, centreline,
lobes: the size query, the class that owns a workspace and the coercion of what `FtpSensor.contacts(K, index_plane=True)` returns."""
from __future__ import annotations

import ctypes
from typing import Optional

import torch

from . import _lib
from ._handle import call


def workspace_bytes(sizer: str, *sizes) -> int:
    """what the library function `sizer` gives for `sizes`; ValueError for sizes the read-out does not take.  Needs no device."""
    n = ctypes.c_size_t()
    call(None, sizer, *(int(v) for v in sizes), ctypes.byref(n))
    return int(n.value)


class Workspace:
    """The device memory of a read-out for up to `batch` frames: one tensor, nothing of the library's.  `_sizer` names the library function
    that sizes it, called with (h, w, batch, *more); `key` is the sizes a call must share with it, (h, w, *more)."""
    _sizer = ""
    h, w, max_contacts = property(lambda self: self.key[0]), property(lambda self: self.key[1]), property(lambda self: self.key[2])

    def __init__(self, device, h: int, w: int, batch: int, *more: int):
        self.key = (int(h), int(w)) + tuple(int(v) for v in more)
        self.batch = int(batch)
        self.device = torch.device(device)
        self.nbytes = workspace_bytes(self._sizer, *self.key[:2], self.batch, *self.key[2:])
        self.buffer: Optional[torch.Tensor] = torch.empty((self.nbytes + 255,), dtype=torch.uint8, device=self.device)

    def fits(self, h: int, w: int, batch: int, *more: int) -> bool:
        return self.buffer is not None and self.key == (int(h), int(w)) + tuple(int(v) for v in more) and int(batch) <= self.batch

    def pointer(self) -> int:
        """the first 256-byte aligned address of the buffer"""
        return (self.buffer.data_ptr() + 255) & ~255

    def close(self):
        self.buffer = None

    @classmethod
    def fitting(cls, given, device, h: int, w: int, batch: int, *more: int):
        """`given` if it is a workspace on `device` that fits these sizes, else one made for the call"""
        return given if given is not None and given.fits(h, w, batch, *more) and given.device == device else cls(h, w, batch, *more, device)


def table_inputs(who: str, contact_index, contacts, count, mm_per_px, device, depth=None, depth_text: str = ""):
    """The opening of `who`, a contact_* function: the device check, then contact_index as [B,h,w] int8 on its own device if it has one,
    else on `device`, and there contacts [B,K,16] float64, count [B] int32, mm_per_px [B] float64 and depth [B,h,w] float32 (None stays
    None; depth_text: its ValueError).  Returns (dev, idx, tab, cnt, mpp, dep, b, h, w, k)."""
    if not torch.cuda.is_available():
        raise RuntimeError(f"{who} needs a HIP device (torch.cuda.is_available() is False); there is no CPU path")
    idx = torch.as_tensor(contact_index)
    dev = idx.device if idx.is_cuda else torch.device(device)
    idx = idx.to(dev, torch.int8).contiguous()
    if idx.dim() != 3:
        raise ValueError("contact_index must be [B,h,w]")
    b, h, w = (int(v) for v in idx.shape)
    tab = torch.as_tensor(contacts).to(dev, torch.float64).contiguous()
    if tab.dim() != 3 or tab.shape[0] != b or tab.shape[2] != _lib.NCONTACT or not 1 <= tab.shape[1] <= _lib.MAX_CONTACTS:
        raise ValueError(f"contacts must be [B,K,{_lib.NCONTACT}] with K in 1..{_lib.MAX_CONTACTS} for the B frames of contact_index")
    cnt, mpp = torch.as_tensor(count).to(dev, torch.int32).contiguous(), torch.as_tensor(mm_per_px).to(dev, torch.float64).contiguous()
    if tuple(cnt.shape) != (b,) or tuple(mpp.shape) != (b,):
        raise ValueError("count and mm_per_px must be [B] for the B frames of contact_index")
    dep = None
    if depth is not None:
        dep = torch.as_tensor(depth).to(dev, torch.float32).contiguous()
        if tuple(dep.shape) != (b, h, w):
            raise ValueError(depth_text)
    return dev, idx, tab, cnt, mpp, dep, b, h, w, int(tab.shape[1])
