"""libdsdtm_amd_motion.so (include/dsdtm_amd_motion.h) from Python: the ctypes binding, and MovingDetector — the shape of the
reference's Moving_Detecter (src/Moving_Detection.cpp) + Frame::Motion_Removal (src/Frame.cpp:342-363) over it.

No fallback: loading raises if the library has not been built, a context raises without a gfx950 device.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _addon

LIB_NAME = "libdsdtm_amd_motion.so"
# every symbol include/dsdtm_amd_motion.h declares
SYMBOLS = ["dsdtm_motion_create", "dsdtm_motion_destroy", "dsdtm_motion_last_error", "dsdtm_motion_model_create",
           "dsdtm_motion_model_destroy", "dsdtm_motion_model_reset", "dsdtm_motion_model_read", "dsdtm_motion_model_write",
           "dsdtm_motion_step", "dsdtm_motion_steps"]
OK, ERR_NO_DEVICE, ERR_INVALID, ERR_HIP, ERR_NOMEM = 0, -1, -2, -3, -4
MIN_SIDE, MAX_SIDE, MAX_FEATURES, STEPS_MAX = 16, 4096, 16384, 1024
ARRAYS = 12


class Desc(C.Structure):
    """dsdtm_motion_desc"""
    _fields_ = [("model", C.c_void_p), ("image", C.c_void_p), ("stride", C.c_int32), ("mask_stride", C.c_int32), ("mask", C.c_void_p),
                ("H", C.c_void_p), ("n_features", C.c_int32), ("reserved", C.c_int32), ("feature_px", C.c_void_p),
                ("feature_on_mask", C.c_void_p)]


class MotionError(RuntimeError):
    def __init__(self, status, message):
        super().__init__(f"status {status}: {message}")
        self.status, self.message = status, message


def lib_path() -> str:
    return _addon.lib_path(LIB_NAME)


def _not_built(path):
    return FileNotFoundError(f"{path} has not been built (python dsdtm_amd/csrc/build.py --all); there is no fallback")


def load():
    """Load libdsdtm_amd_motion.so. Raises if it has not been built (dsdtm_amd/csrc/build.py --all)."""
    vp, i = C.c_void_p, C.c_int
    return _addon.load_addon(LIB_NAME, {
        **_addon.context_signatures("dsdtm_motion"), "dsdtm_motion_model_create": (i, [vp, i, i, C.POINTER(vp)]),
        "dsdtm_motion_model_destroy": (None, [vp, vp]), "dsdtm_motion_model_reset": (i, [vp, vp]),
        "dsdtm_motion_model_read": (i, [vp, vp, vp]), "dsdtm_motion_model_write": (i, [vp, vp, vp]),
        "dsdtm_motion_step": (i, [vp, vp, vp, i, vp, vp, i, i, vp, vp]), "dsdtm_motion_steps": (i, [vp, i, C.POINTER(Desc)])}, _not_built)


class MotionContext(_addon.AddonContext):
    """A dsdtm_motion_ctx: its own stream and staging block on one device. One per calling thread."""
    PREFIX, ERROR, load = "dsdtm_motion", MotionError, staticmethod(load)

    def prepare(self, steps) -> "PreparedSteps":
        """A dsdtm_motion_steps call built once (descriptors, output arrays), to be run any number of times."""
        return PreparedSteps(self, steps)

    def steps(self, steps) -> list:
        """dsdtm_motion_steps: `steps` is a list of dicts(model, image, H, want_mask=True, features=None, stride=None). One
        submission. Returns one (mask or None, flags or None) per entry. image: a uint8 numpy array (h x w, rows may be strided) or
        anything with data_ptr() / stride() on this device (a torch tensor)."""
        p = PreparedSteps(self, steps)
        self.check(p.run_raw())
        return p.outs


class PreparedSteps:
    """The descriptors of one dsdtm_motion_steps call and every array they point at; run_raw() is the C call alone."""

    def __init__(self, ctx, steps):
        self.ctx, self.n = ctx, len(steps)
        self.descs = (Desc * max(self.n, 1))()
        self.keep, self.outs = [], []
        for k, s in enumerate(steps):
            m = s["model"]
            ptr, stride, hold = _image_pointer(s["image"], m.width, m.height, s.get("stride"))
            H = np.ascontiguousarray(np.asarray(s["H"], np.float64).reshape(9))
            mask = np.full((m.height, m.width), 0xA5, np.uint8) if s.get("want_mask", True) else None
            f = s.get("features")
            f = None if f is None else np.ascontiguousarray(np.asarray(f, np.float32).reshape(-1, 2))
            flags = None if f is None else np.full(len(f), 0xA5, np.uint8)
            self.keep.append((hold, H, f, m))
            self.outs.append((mask, flags))
            d = self.descs[k]
            d.model, d.image, d.stride, d.H = m.handle, ptr, stride, H.ctypes.data
            d.mask, d.mask_stride = (mask.ctypes.data, m.width) if mask is not None else (None, 0)
            d.n_features = 0 if f is None else len(f)
            d.feature_px = f.ctypes.data if f is not None and len(f) else None
            d.feature_on_mask = flags.ctypes.data if flags is not None and len(flags) else None

    def run_raw(self) -> int:
        return self.ctx.lib.dsdtm_motion_steps(self.ctx.handle, self.n, self.descs)


def _image_pointer(image, width, height, stride=None):
    if isinstance(image, np.ndarray):
        if image.dtype != np.uint8 or image.shape != (height, width) or image.strides[1] != 1:
            raise ValueError(f"image must be uint8 {height} x {width} with contiguous rows")
        return image.ctypes.data, image.strides[0] if stride is None else stride, image
    if hasattr(image, "data_ptr"):          # a device tensor, read where it is
        if tuple(image.shape) != (height, width) or image.stride(1) != 1:
            raise ValueError(f"image must be uint8 {height} x {width} with contiguous rows")
        return image.data_ptr(), image.stride(0) if stride is None else stride, image
    return int(image), int(stride), None    # a raw address (tests of the argument checks)


class MotionModel:
    """A dsdtm_motion_model: the device-resident ProbModel of one tracker (ProbModel::init done)."""

    def __init__(self, ctx: MotionContext, width: int, height: int):
        self.ctx, self.width, self.height = ctx, int(width), int(height)
        self.mw, self.mh = self.width // 4, self.height // 4
        h = C.c_void_p()
        ctx.check(ctx.lib.dsdtm_motion_model_create(ctx.handle, self.width, self.height, C.byref(h)))
        self.handle = h

    def close(self):
        if getattr(self, "handle", None) and getattr(self.ctx, "handle", None):
            self.ctx.lib.dsdtm_motion_model_destroy(self.ctx.handle, self.handle)
        self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def reset(self):
        self.ctx.check(self.ctx.lib.dsdtm_motion_model_reset(self.ctx.handle, self.handle))

    def read(self) -> np.ndarray:
        """(12, cells) float32: m_Mean, m_Var, m_Age, m_Mean_Temp, m_Var_Temp, m_Age_Temp x 2 modes."""
        out = np.empty((ARRAYS, self.mw * self.mh), np.float32)
        self.ctx.check(self.ctx.lib.dsdtm_motion_model_read(self.ctx.handle, self.handle, out.ctypes.data))
        return out

    def write(self, state):
        st = np.ascontiguousarray(np.asarray(state, np.float32).reshape(ARRAYS, self.mw * self.mh))
        self.ctx.check(self.ctx.lib.dsdtm_motion_model_write(self.ctx.handle, self.handle, st.ctypes.data))

    def step(self, image, H, want_mask=True, features=None, stride=None):
        """dsdtm_motion_step (the single entry). Returns (mask or None, flags or None)."""
        ptr, stride, hold = _image_pointer(image, self.width, self.height, stride)
        H = np.ascontiguousarray(np.asarray(H, np.float64).reshape(9))
        mask = np.full((self.height, self.width), 0xA5, np.uint8) if want_mask else None
        f = None if features is None else np.ascontiguousarray(np.asarray(features, np.float32).reshape(-1, 2))
        flags = None if f is None else np.full(len(f), 0xA5, np.uint8)
        st = self.ctx.lib.dsdtm_motion_step(self.ctx.handle, self.handle, ptr, stride, H.ctypes.data,
                                            mask.ctypes.data if mask is not None else None, self.width if mask is not None else 0,
                                            0 if f is None else len(f), f.ctypes.data if f is not None and len(f) else None,
                                            flags.ctypes.data if flags is not None and len(flags) else None)
        del hold
        self.ctx.check(st)
        return mask, flags


class MovingDetector:
    """Moving_Detecter (src/Moving_Detection.cpp) + Frame::Motion_Removal (src/Frame.cpp:342-363) over the C ABI.

    Mod_FastMCD(image, H) is MCDWrapper::Run up to BGModel.update(detect_img): the mask BEFORE the contour step (out of scope, see the
    header). H is the caller's cv::findHomography(tPointsA, tPointsB, CV_RANSAC). The model is created on the first image, as
    MCDWrapper::Run does at frm_cnt == 0.
    required_rows: Tracking::MotionRemoval returns early unless the image has 480 rows (src/Tracking.cpp:509); here that is a
    parameter (None: no such test) and an image of another height raises.
    Note that the reference's call of MotionRemoval is commented out (src/Tracking.cpp:230)."""

    def __init__(self, ctx: MotionContext | None = None, required_rows: int | None = None, device: int = 0):
        self.ctx = ctx or MotionContext(device)
        self.required_rows = required_rows
        self.model = None
        self.mask = None
        self._pending = None

    def Mod_FastMCD(self, image, H, features=None) -> np.ndarray:
        h, w = int(image.shape[0]), int(image.shape[1])
        if self.required_rows is not None and h != self.required_rows:
            raise ValueError(f"image has {h} rows, not {self.required_rows} (src/Tracking.cpp:509)")
        if self.model is None:
            self.model = MotionModel(self.ctx, w, h)
        self.mask, flags = self.model.step(image, H, want_mask=True, features=features)
        self._pending = flags
        return self.mask

    def motion_removal(self, features):
        """Frame::Motion_Removal against the last mask: returns (keep, rebuilt). keep[i] = 1 when feature i does not lie on the mask
        (:352: mask.at(cvRound(x), cvRound(y)) != 255). rebuilt is the list the reference actually ends with: it starts tmpFeatures
        as a COPY of all features and then appends the kept ones again (src/Frame.cpp:346-356), so every feature survives and the
        kept ones appear twice — rebuilt holds indices into `features`: 0 .. n-1, then the kept ones in order.
        The lookup ran on the device, against the mask where it lay, in the submission of the last Mod_FastMCD: `features` must be
        the ones that call was given (there is no host lookup to fall back to)."""
        f = np.asarray(features, np.float32).reshape(-1, 2)
        if self._pending is None or len(self._pending) != len(f):
            raise RuntimeError("motion_removal needs the features the last Mod_FastMCD was given")
        keep = (np.asarray(self._pending) == 0).astype(np.uint8)
        rebuilt = list(range(len(f))) + [int(k) for k in np.flatnonzero(keep)]
        return keep, rebuilt
