"""libdsdtm_amd_mcd.so (include/dsdtm_amd_mcd.h) from Python: the ctypes binding, and MotionDetector — the reference's Moving_Detecter
(src/Moving_Detection.cpp) + Frame::Motion_Removal (src/Frame.cpp:342-363) with Mod_FastMCD as the WHOLE MCDWrapper::Run, contour box
included. dsdtm_amd/motion.py is the same up to BGModel.update(detect_img) and stays as it is; a model belongs to the context that
made it, so a process that wants the whole Run keeps its models here.

No fallback: loading raises if the library has not been built, a context raises without a gfx950 device.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _addon
from .motion import ARRAYS, _image_pointer

LIB_NAME = "libdsdtm_amd_mcd.so"
# every symbol include/dsdtm_amd_mcd.h declares
SYMBOLS = ["dsdtm_mcd_create", "dsdtm_mcd_destroy", "dsdtm_mcd_last_error", "dsdtm_mcd_model_create", "dsdtm_mcd_model_destroy",
           "dsdtm_mcd_model_reset", "dsdtm_mcd_model_read", "dsdtm_mcd_model_write", "dsdtm_mcd_steps", "dsdtm_mcd_step", "dsdtm_mcd_boxes"]
OK, ERR_NO_DEVICE, ERR_INVALID, ERR_HIP, ERR_NOMEM = 0, -1, -2, -3, -4
MIN_SIDE, MAX_SIDE, MAX_FEATURES, STEPS_MAX, MAX_PIXELS = 16, 4096, 16384, 1024, 1 << 20


class Desc(C.Structure):
    """dsdtm_mcd_desc"""
    _fields_ = [("model", C.c_void_p), ("image", C.c_void_p), ("stride", C.c_int32), ("mask_stride", C.c_int32), ("mask", C.c_void_p),
                ("H", C.c_void_p), ("n_features", C.c_int32), ("mask_raw_stride", C.c_int32), ("feature_px", C.c_void_p),
                ("feature_on_mask", C.c_void_p), ("mask_raw", C.c_void_p), ("box", C.c_int32 * 4), ("area2", C.c_int64),
                ("n_components", C.c_int32), ("reserved", C.c_int32)]


class BoxDesc(C.Structure):
    """dsdtm_mcd_box_desc"""
    _fields_ = [("mask", C.c_void_p), ("width", C.c_int32), ("height", C.c_int32), ("stride", C.c_int32), ("boxed_stride", C.c_int32),
                ("boxed", C.c_void_p), ("box", C.c_int32 * 4), ("area2", C.c_int64), ("n_components", C.c_int32), ("reserved", C.c_int32)]


class McdError(RuntimeError):
    def __init__(self, status, message):
        super().__init__(f"status {status}: {message}")
        self.status, self.message = status, message


def lib_path() -> str:
    return _addon.lib_path(LIB_NAME)


def _not_built(path):
    return FileNotFoundError(f"{path} has not been built (python dsdtm_amd/csrc/build.py --all); there is no fallback")


def load():
    """Load libdsdtm_amd_mcd.so. Raises if it has not been built (dsdtm_amd/csrc/build.py --all)."""
    vp, i = C.c_void_p, C.c_int
    return _addon.load_addon(LIB_NAME, {
        **_addon.context_signatures("dsdtm_mcd"), "dsdtm_mcd_model_create": (i, [vp, i, i, C.POINTER(vp)]),
        "dsdtm_mcd_model_destroy": (None, [vp, vp]), "dsdtm_mcd_model_reset": (i, [vp, vp]),
        "dsdtm_mcd_model_read": (i, [vp, vp, vp]), "dsdtm_mcd_model_write": (i, [vp, vp, vp]),
        "dsdtm_mcd_steps": (i, [vp, i, C.POINTER(Desc)]),
        "dsdtm_mcd_step": (i, [vp, vp, vp, i, vp, vp, i, vp, i, i, vp, vp, vp, vp, vp]),
        "dsdtm_mcd_boxes": (i, [vp, i, C.POINTER(BoxDesc)])}, _not_built)


class McdContext(_addon.AddonContext):
    """A dsdtm_mcd_ctx: its own stream and staging block on one device. One per calling thread."""
    PREFIX, ERROR, load = "dsdtm_mcd", McdError, staticmethod(load)

    def prepare(self, steps) -> "PreparedSteps":
        """A dsdtm_mcd_steps call built once (descriptors, output arrays), to be run any number of times."""
        return PreparedSteps(self, steps)

    def steps(self, steps) -> list:
        """dsdtm_mcd_steps: `steps` is a list of dicts(model, image, H, want_mask=True, want_raw=False, features=None, stride=None). One
        submission. Returns one dict(mask, mask_raw, flags, box, area2, n_components) per entry (what was not wanted is None)."""
        p = PreparedSteps(self, steps)
        self.check(p.run_raw())
        return p.results()

    def boxes(self, masks, want_boxed=True) -> list:
        """dsdtm_mcd_boxes: rules C1-C5 on 8-bit masks — uint8 numpy arrays (rows may be strided), anything with data_ptr() / stride()
        on this device (a torch tensor), or dict(ptr, width, height, stride) (tests of the argument checks). One submission.
        Returns one dict(box, area2, n_components, boxed) per mask."""
        n = len(masks)
        descs = (BoxDesc * max(n, 1))()
        keep, outs = [], []
        for k, m in enumerate(masks):
            d = descs[k]
            if isinstance(m, dict):
                d.mask, d.width, d.height, d.stride = m["ptr"], m["width"], m["height"], m["stride"]
            elif isinstance(m, np.ndarray):
                if m.dtype != np.uint8 or m.ndim != 2 or m.strides[1] != 1:
                    raise ValueError("a mask must be a 2-d uint8 array with contiguous rows")
                d.mask, d.width, d.height, d.stride = m.ctypes.data, m.shape[1], m.shape[0], m.strides[0]
            else:
                d.mask, d.width, d.height, d.stride = m.data_ptr(), int(m.shape[1]), int(m.shape[0]), m.stride(0)
            boxed = np.full((d.height, d.width), 0xA5, np.uint8) if want_boxed and 0 < d.height <= MAX_SIDE and 0 < d.width <= MAX_SIDE else None
            if boxed is not None:
                d.boxed, d.boxed_stride = boxed.ctypes.data, d.width
            keep.append(m)
            outs.append(boxed)
        self.check(self.lib.dsdtm_mcd_boxes(self.handle, n, descs))
        del keep
        return [dict(box=list(descs[k].box), area2=int(descs[k].area2), n_components=int(descs[k].n_components), boxed=outs[k]) for k in range(n)]


class PreparedSteps:
    """The descriptors of one dsdtm_mcd_steps call and every array they point at; run_raw() is the C call alone."""

    def __init__(self, ctx, steps):
        self.ctx, self.n = ctx, len(steps)
        self.descs = (Desc * max(self.n, 1))()
        self.keep, self.outs = [], []
        for k, s in enumerate(steps):
            m = s["model"]
            ptr, stride, hold = _image_pointer(s["image"], m.width, m.height, s.get("stride"))
            H = np.ascontiguousarray(np.asarray(s["H"], np.float64).reshape(9))
            mask = np.full((m.height, m.width), 0xA5, np.uint8) if s.get("want_mask", True) else None
            raw = np.full((m.height, m.width), 0xA5, np.uint8) if s.get("want_raw", False) else None
            f = s.get("features")
            f = None if f is None else np.ascontiguousarray(np.asarray(f, np.float32).reshape(-1, 2))
            flags = None if f is None else np.full(len(f), 0xA5, np.uint8)
            self.keep.append((hold, H, f, m))
            self.outs.append((mask, raw, flags))
            d = self.descs[k]
            d.model, d.image, d.stride, d.H = m.handle, ptr, stride, H.ctypes.data
            d.mask, d.mask_stride = (mask.ctypes.data, m.width) if mask is not None else (None, 0)
            d.mask_raw, d.mask_raw_stride = (raw.ctypes.data, m.width) if raw is not None else (None, 0)
            d.n_features = 0 if f is None else len(f)
            d.feature_px = f.ctypes.data if f is not None and len(f) else None
            d.feature_on_mask = flags.ctypes.data if flags is not None and len(flags) else None
            d.box[:] = [-1, -1, -1, -1]
            d.area2, d.n_components = -1, -1

    def run_raw(self) -> int:
        return self.ctx.lib.dsdtm_mcd_steps(self.ctx.handle, self.n, self.descs)

    def results(self) -> list:
        return [dict(mask=o[0], mask_raw=o[1], flags=o[2], box=list(self.descs[k].box), area2=int(self.descs[k].area2),
                     n_components=int(self.descs[k].n_components)) for k, o in enumerate(self.outs)]


class McdModel:
    """A dsdtm_mcd_model: the device-resident ProbModel of one tracker (ProbModel::init done), in an mcd context."""

    def __init__(self, ctx: McdContext, width: int, height: int):
        self.ctx, self.width, self.height = ctx, int(width), int(height)
        self.mw, self.mh = self.width // 4, self.height // 4
        h = C.c_void_p()
        ctx.check(ctx.lib.dsdtm_mcd_model_create(ctx.handle, self.width, self.height, C.byref(h)))
        self.handle = h

    def close(self):
        if getattr(self, "handle", None) and getattr(self.ctx, "handle", None):
            self.ctx.lib.dsdtm_mcd_model_destroy(self.ctx.handle, self.handle)
        self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def reset(self):
        self.ctx.check(self.ctx.lib.dsdtm_mcd_model_reset(self.ctx.handle, self.handle))

    def read(self) -> np.ndarray:
        """(12, cells) float32: m_Mean, m_Var, m_Age, m_Mean_Temp, m_Var_Temp, m_Age_Temp x 2 modes."""
        out = np.empty((ARRAYS, self.mw * self.mh), np.float32)
        self.ctx.check(self.ctx.lib.dsdtm_mcd_model_read(self.ctx.handle, self.handle, out.ctypes.data))
        return out

    def write(self, state):
        st = np.ascontiguousarray(np.asarray(state, np.float32).reshape(ARRAYS, self.mw * self.mh))
        self.ctx.check(self.ctx.lib.dsdtm_mcd_model_write(self.ctx.handle, self.handle, st.ctypes.data))

    def step(self, image, H, want_mask=True, want_raw=False, features=None, stride=None) -> dict:
        """dsdtm_mcd_step (the single entry): dict(mask, mask_raw, flags, box, area2, n_components)."""
        ptr, stride, hold = _image_pointer(image, self.width, self.height, stride)
        H = np.ascontiguousarray(np.asarray(H, np.float64).reshape(9))
        mask = np.full((self.height, self.width), 0xA5, np.uint8) if want_mask else None
        raw = np.full((self.height, self.width), 0xA5, np.uint8) if want_raw else None
        f = None if features is None else np.ascontiguousarray(np.asarray(features, np.float32).reshape(-1, 2))
        flags = None if f is None else np.full(len(f), 0xA5, np.uint8)
        box, area2, count = (C.c_int32 * 4)(-1, -1, -1, -1), C.c_int64(-1), C.c_int32(-1)
        st = self.ctx.lib.dsdtm_mcd_step(self.ctx.handle, self.handle, ptr, stride, H.ctypes.data,
                                         raw.ctypes.data if raw is not None else None, self.width if raw is not None else 0,
                                         mask.ctypes.data if mask is not None else None, self.width if mask is not None else 0,
                                         0 if f is None else len(f), f.ctypes.data if f is not None and len(f) else None,
                                         flags.ctypes.data if flags is not None and len(flags) else None,
                                         C.cast(box, C.c_void_p), C.cast(C.pointer(area2), C.c_void_p), C.cast(C.pointer(count), C.c_void_p))
        del hold
        self.ctx.check(st)
        return dict(mask=mask, mask_raw=raw, flags=flags, box=list(box), area2=int(area2.value), n_components=int(count.value))


class MotionDetector:
    """Moving_Detecter (src/Moving_Detection.cpp) + Frame::Motion_Removal (src/Frame.cpp:342-363) over the C ABI, with the shape of
    dsdtm_amd.motion.MovingDetector. Run(image, H) is the WHOLE MCDWrapper::Run (Thirdparty/fastMCD/src/MCDWrapper.cpp:65-137): the
    returned image has the bounding rectangle of the largest contour filled in (rules C1-C5 of the header) and the feature flags are
    looked up on it (C6), which is what the reference's Motion_Removal reads. Mod_FastMCD is Run under Moving_Detecter's name."""

    def __init__(self, ctx: McdContext | None = None, required_rows: int | None = None, device: int = 0):
        self.ctx = ctx or McdContext(device)
        self.required_rows = required_rows
        self.model = None
        self.mask = self.mask_raw = self.box = None
        self.area2 = self.n_components = 0
        self._pending = None

    def Run(self, image, H, features=None, want_raw=False) -> np.ndarray:
        h, w = int(image.shape[0]), int(image.shape[1])
        if self.required_rows is not None and h != self.required_rows:
            raise ValueError(f"image has {h} rows, not {self.required_rows} (src/Tracking.cpp:509)")
        if self.model is None:
            self.model = McdModel(self.ctx, w, h)
        r = self.model.step(image, H, want_mask=True, want_raw=want_raw, features=features)
        self.mask, self.mask_raw, self.box, self.area2, self.n_components = r["mask"], r["mask_raw"], r["box"], r["area2"], r["n_components"]
        self._pending = r["flags"]
        return self.mask

    Mod_FastMCD = Run

    def RunTrack(self, image, features=None, want_raw=False) -> np.ndarray:
        """Run without an H argument, as MCDWrapper::Run works: a KLTWrapper (dsdtm_amd/klt.py, libdsdtm_amd_klt.so; made on first use,
        on this detector's device) tracks its grid from the last image into this one, and its H goes into Run. The first image seeds
        it (identity). self.klt.last holds the step's result (source, n_tracked, n_inliers)."""
        if getattr(self, "klt", None) is None:
            from . import klt as _klt
            self.klt = _klt.KLTWrapper(device=self.ctx.device)
        self.klt.RunTrack(image)
        return self.Run(image, self.klt.GetHomography().reshape(9), features=features, want_raw=want_raw)

    def _framediff(self, a, b, H, flags, features, threshold, maxval):
        if getattr(self, "framediff", None) is None:
            from . import framediff as _fd
            self.framediff = _fd.FrameDiffContext(self.ctx.device)
        r = self.framediff.step(a, b, H, flags=flags, threshold=threshold, maxval=maxval, features=features)
        self.mask, self.last_framediff = r["mask"], r
        self._pending = r["flags"]
        return self.mask

    def Mod_FrameDiff(self, image_a, image_b, points_a, points_b, features=None, threshold=50, maxval=0):
        """Moving_Detecter::Mod_FrameDiff (src/Moving_Detection.cpp:36-63) over libdsdtm_amd_homography.so and libdsdtm_amd_framediff.so
        (contexts made on first use, on this detector's device): H = dsdtm_find_homography(points_b, points_a), image_b warped by it,
        image_a - warped, threshold, open, dilate. Fewer than 4 points: None (:40-41); so is a fit that finds nothing.
        image_b IS FRAME B: the reference's :45 passes frame A twice (QUIRK 1 of the header); a caller who wants that passes image_a for
        both. maxval 0 is the reference's 200, at which motion_removal removes nothing (QUIRK 2); 255 makes the mask act."""
        pa, pb = np.asarray(points_a, np.float32).reshape(-1, 2), np.asarray(points_b, np.float32).reshape(-1, 2)
        if len(pa) < 4:
            return None
        if getattr(self, "homography", None) is None:
            from . import homography as _h
            self.homography = _h.HomographyContext(self.ctx.device)
        fit = self.homography.find_homography(pb, pa)
        if fit["found"] != 1:
            return None
        return self._framediff(image_a, image_b, fit["H"], 0, features, threshold, maxval)

    def Mod_FrameDiff_KLT(self, image, features=None, threshold=50, maxval=0):
        """Mod_FrameDiff from images alone: a KLTWrapper (dsdtm_amd/klt.py; made on first use) tracks its grid from the last image into
        this one; its H maps the current frame to the last one, which is the map's own direction, so it goes in with INVERSE_MAP, a the
        current image and b the previous one. The first image seeds the tracker and returns None."""
        if getattr(self, "klt", None) is None:
            from . import klt as _klt
            self.klt = _klt.KLTWrapper(device=self.ctx.device)
        prev = getattr(self, "_framediff_prev", None)
        self.klt.RunTrack(image)
        self._framediff_prev = image.clone() if hasattr(image, "clone") else np.array(image, np.uint8)      # a copy: the caller may refill its buffer
        if prev is None:
            return None
        from . import framediff as _fd
        return self._framediff(image, prev, self.klt.GetHomography().reshape(9), _fd.INVERSE_MAP, features, threshold, maxval)

    def motion_removal(self, features):
        """Frame::Motion_Removal against the last image Run returned: (keep, rebuilt), as dsdtm_amd.motion.MovingDetector.motion_removal."""
        f = np.asarray(features, np.float32).reshape(-1, 2)
        if self._pending is None or len(self._pending) != len(f):
            raise RuntimeError("motion_removal needs the features the last Run was given")
        keep = (np.asarray(self._pending) == 0).astype(np.uint8)
        rebuilt = list(range(len(f))) + [int(k) for k in np.flatnonzero(keep)]
        return keep, rebuilt
