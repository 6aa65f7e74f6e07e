"""What the ctypes bindings of the add-on libraries (capi: libdsdtm_amd_keyframe.so, motion: libdsdtm_amd_motion.so,
homography: libdsdtm_amd_homography.so) share: the loader and the context. No fallback: loading raises if the library has not been built, a context raises without a gfx950 device."""
from __future__ import annotations

import ctypes as C
import os

OK = 0
_LIBS = {}


def lib_path(lib_name: str) -> str:
    return os.path.join(os.path.dirname(os.path.abspath(__file__)), "csrc", lib_name)


def load_addon(lib_name: str, signatures: dict, not_built=None):
    """The library csrc/<lib_name> with `signatures` (name -> (restype, argtypes)) attached; loaded once. `not_built(path)` makes the
    exception for a library that is not there."""
    lib = _LIBS.get(lib_name)
    if lib is None:
        path = lib_path(lib_name)
        if not os.path.exists(path):
            raise (not_built or FileNotFoundError)(path)
        lib = C.CDLL(path)
        for name, (res, args) in signatures.items():
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = res, args
        _LIBS[lib_name] = lib
    return lib


def context_signatures(prefix: str) -> dict:
    """<prefix>_create / _destroy / _last_error: the entries every add-on has (csrc/addon_host.h)."""
    return {prefix + "_create": (C.c_int, [C.c_int, C.POINTER(C.c_void_p)]), prefix + "_destroy": (None, [C.c_void_p]),
            prefix + "_last_error": (C.c_char_p, [C.c_void_p])}


class AddonContext:
    """An add-on's context (its own stream and staging block on one device; one per calling thread). A subclass names PREFIX (the
    symbols are PREFIX_create, PREFIX_destroy, PREFIX_last_error), ERROR (raised as ERROR(status, message)) and load() (the library)."""
    PREFIX = ERROR = None

    @staticmethod
    def load():
        raise NotImplementedError

    def __init__(self, device: int = 0):
        self.lib = self.load()
        self.device = device
        h = C.c_void_p()
        st = self._fn("create")(device, C.byref(h))
        if st != OK:
            raise self.ERROR(st, (self._fn("last_error")(None) or b"").decode())
        self.handle = h

    def _fn(self, name):
        return getattr(self.lib, f"{self.PREFIX}_{name}")

    def last_error(self) -> str:
        return (self._fn("last_error")(self.handle) or b"").decode()

    def check(self, st: int):
        if st != OK:
            raise self.ERROR(st, self.last_error())

    def close(self):
        if getattr(self, "handle", None):
            self._fn("destroy")(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
