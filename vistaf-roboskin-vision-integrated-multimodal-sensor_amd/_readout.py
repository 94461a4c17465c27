"""What the read-out classes share: the library handle's life, the device check, the stream and the coercion of an argument."""
from __future__ import annotations

import ctypes

import torch

from . import _lib


class Readout:
    """Base of the classes that wrap one handle of the C ABI.  `_destroy` names the library function that frees the handle."""
    _destroy = ""

    def _open(self, device, need_device: bool = True):
        """the library, an empty handle for the create call to fill, the device"""
        self._lib = _lib.load()
        self._h = ctypes.c_void_p()
        if need_device:
            self._need_device()
        self.device = torch.device(device)

    def _need_device(self, what: str = ""):
        if not torch.cuda.is_available():
            raise RuntimeError(f"{type(self).__name__}{'.' + what if what else ''} needs a HIP device (torch.cuda.is_available() is False); "
                               "there is no CPU path")

    def _stream(self) -> int:
        return int(torch.cuda.current_stream(self.device).cuda_stream)

    def _t(self, value, dtype, shape=None, message: str = ""):
        """value as a contiguous tensor of `dtype` on the device; None stays None.  shape: what it must be, None as its first entry for
        any batch; ValueError(message) otherwise."""
        if value is None:
            return None
        t = torch.as_tensor(value).to(self.device, dtype).contiguous()
        if shape is not None and t.shape != shape and (shape[0] is not None or t.dim() != len(shape) or t.shape[1:] != shape[1:]):
            raise ValueError(message)
        return t

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            getattr(self._lib, self._destroy)(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def ptr(t):
    return None if t is None else t.data_ptr()
