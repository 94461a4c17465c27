"""What the classes that wrap a handle of the C ABI share: the handle's life, the device check, the stream, the one way to call the library
and the coercion of an argument."""
from __future__ import annotations

import contextlib
import ctypes

import torch

from . import _lib


def stream(device) -> int:
    """the current stream of `device`, as the `void *stream` argument of the ABI"""
    return int(torch.cuda.current_stream(device).cuda_stream)


def call(device, name: str, *args):
    """The library function `name` with `device` current, or as things are for device None (a function that touches no device: argument
    checks, host tables, flags -- these also run where there is no device).  A return other than 0 raises with the library's last-error
    text (ValueError for VISTAF_E_INVALID, RuntimeError otherwise)."""
    with torch.cuda.device(device) if device is not None else contextlib.nullcontext():
        _lib.check(getattr(_lib.load(), name)(*args))


class Handle:
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
        return stream(self.device)

    def _call(self, name: str, *args, on_device: bool = True):
        call(self.device if on_device else None, name, *args)

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
