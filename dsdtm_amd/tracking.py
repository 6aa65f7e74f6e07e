"""One tracked frame of DSDTM::Tracking (reference src/Tracking.cpp:199-256) through ONE library call — the host mirror
of dsdtm_track_frame, with the side effects the reference's classes leave on the frame and the map:

    TrackWithLastFrame   cur.Set_Pose(last.Get_Pose()); Sprase_ImgAlign::Run(cur, last)                  (:199-217)
    UpdateLocalMap       ResetGrid; ReprojectPoint for every local map point                              (:258-312)
    TrackWithLocalMap    SearchLocalPoints(cur) (new Features, IncreaseFound, mask discs);
                         Optimizer::PoseOptimization(cur) (Set_Pose, the EraseFound walk)                 (:219-256)

The four-call chain (sparse_align.Sprase_ImgAlign, search.LocalPointSearch, optimizer.Optimizer on device-resident frames)
does the same with a host round trip between the steps; tests hold the two to the same bits. No CPU path: the library call
fails loudly without the HIP library or a gfx950 device.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import capi, search
from .frame import Config, Frame
from .keyframe_decision import KeyframeParams


def flatten_local_map(keyframes, map_points):
    """The local map as dsdtm_track_desc wants it: map-point columns + observations in CSR form (iteration order of
    mObservations = keyframe-index order, as search.get_closest_obs walks it), each observation carrying the observing
    feature's mpx / mlevel / mNormal."""
    M = len(map_points)
    pw = np.zeros((M, 3), np.float64)
    found = np.zeros(M, np.int32)
    bad = np.zeros(M, np.uint8)
    off = np.zeros(M + 1, np.int32)
    okf, ofe = [], []
    for i, mp in enumerate(map_points):
        pw[i] = mp.Get_Pose()
        found[i] = mp.Get_FoundNums()
        bad[i] = 1 if mp.IsBad() else 0
        for k in sorted(mp.mObservations):
            okf.append(k)
            ofe.append(mp.mObservations[k])
        off[i + 1] = len(okf)
    okf = np.array(okf, np.int32)
    n = len(okf)
    opx, olv, ob = np.zeros((n, 2), np.float32), np.zeros(n, np.int32), np.zeros((n, 3), np.float64)
    for j in range(n):
        kf = keyframes[int(okf[j])]
        opx[j], olv[j], ob[j] = kf.px[ofe[j]], kf.level[ofe[j]], kf.bearing[ofe[j]]
    return dict(pw=pw, found=found, bad=bad, off=off, okf=okf, opx=opx, olv=olv, ob=ob)


class TrackCall:
    """One prepared dsdtm_track_frame call: the descriptor and every array it points at are built once (`__init__`), `run()`
    is the library call alone — what a C++ Tracking pays per frame (bench_tracking.py times it; a frame's release is the
    caller's: result["frame"].close()). With `cur_frame` (a capi.DeviceFrame from DeviceFrame.prefetch or .from_image) the call is
    dsdtm_track_frame_on: the new frame is already on the device, or on its way there, `image` is not read (it may be None) and
    result["frame"] is cur_frame."""

    def __init__(self, ctx: capi.Context, cam, image, levels, last: Frame, T_seed, align, min_tracked, keyframes, map_points,
                 mask=None, cell_size=None, max_pyr_levels=None, max_matches=200, align2d_iters=10, po_iterations=100, flat=None,
                 cur_frame=None):
        self.ctx = ctx
        self.cur_frame = cur_frame
        if cur_frame is not None:
            image = np.zeros((0, 0), np.uint8)                 # (never read: the descriptor's image stays NULL)
        image = np.asarray(image)
        if cur_frame is None and (image.dtype != np.uint8 or image.ndim != 2 or image.strides[1] != 1 or image.strides[0] < image.shape[1]):
            image = np.ascontiguousarray(image, np.uint8)      # (a row-strided uint8 view goes down as it is: d.stride)
        cell_size = int(Config.Get("Camera.CellSize") if cell_size is None else cell_size)
        max_pyr_levels = int(Config.Get("Camera.MaxPyraLevels") if max_pyr_levels is None else max_pyr_levels)
        fm = flat if flat is not None else flatten_local_map(keyframes, map_points)
        d = capi.TrackDesc()
        if cur_frame is None:
            d.image, d.width, d.height, d.stride, d.levels = image.ctypes.data, image.shape[1], image.shape[0], image.strides[0], int(levels)
        else:
            d.image, d.width, d.height, d.stride, d.levels = None, cam.width, cam.height, cam.width, int(levels)
        dref = capi.device_frame_of(ctx, last)
        d.ref = dref.handle
        px = np.ascontiguousarray(last.px, np.float32)
        bear, pw, ini = np.ascontiguousarray(last.bearing), np.ascontiguousarray(last.p_world), np.ascontiguousarray(last.initial, np.uint8)
        d.ref_px_xy, d.ref_bearing, d.ref_p_world, d.ref_initial = px.ctypes.data, bear.ctypes.data, pw.ctypes.data, ini.ctypes.data
        d.n_ref_features = last.n_features
        Tr = np.ascontiguousarray(last.Get_Pose(), np.float64).reshape(12).copy()
        Ts = np.ascontiguousarray(T_seed, np.float64).reshape(12).copy()
        d.T_ref_w, d.T_seed = Tr.ctypes.data, Ts.ctypes.data
        d.align = capi.AlignParams(*[int(v) for v in align])
        d.min_tracked = int(min_tracked)
        kfd = [capi.device_frame_of(ctx, k) for k in keyframes]
        kfh = (C.c_void_p * max(1, len(keyframes)))(*[k.handle for k in kfd])
        Tk = np.ascontiguousarray(np.array([k.Get_Pose() for k in keyframes], np.float64).reshape(len(keyframes), 12))
        d.kf, d.n_kf, d.T_kf_w = C.cast(kfh, C.c_void_p), len(keyframes), Tk.ctypes.data
        d.n_points = len(fm["found"])
        d.mp_world, d.mp_found, d.mp_bad, d.obs_offset = fm["pw"].ctypes.data, fm["found"].ctypes.data, fm["bad"].ctypes.data, fm["off"].ctypes.data
        d.obs_kf, d.obs_px, d.obs_level, d.obs_bearing = fm["okf"].ctypes.data, fm["opx"].ctypes.data, fm["olv"].ctypes.data, fm["ob"].ctypes.data
        if mask is not None:
            mask = np.ascontiguousarray(mask, np.uint8)
            d.mask, d.mask_stride = mask.ctypes.data, mask.strides[0]
        d.cell_size, d.max_pyr_levels, d.max_matches, d.align2d_iters = cell_size, max_pyr_levels, int(max_matches), int(align2d_iters)
        d.pose_opt = capi.PoseOptParams(int(po_iterations), 0)
        self.desc = d
        self.res = capi.TrackResult()
        self.matches = np.zeros(max(1, int(max_matches)), capi.TRACK_MATCH_DTYPE)
        self.rn = np.zeros(max(1, int(max_matches)))
        self.cs = capi.camera_struct(cam)
        self._keep = (image, dref, px, bear, pw, ini, Tr, Ts, kfd, kfh, Tk, fm, mask)

    def run_raw(self) -> int:
        """The library call alone; returns its status (the new frame's handle is in self.res.frame)."""
        if self.cur_frame is not None:
            return self.ctx.lib.dsdtm_track_frame_on(self.ctx.handle, C.byref(self.cs), C.byref(self.desc), self.cur_frame.handle,
                                                     C.byref(self.res), self.matches.ctypes.data, self.rn.ctypes.data)
        return self.ctx.lib.dsdtm_track_frame(self.ctx.handle, C.byref(self.cs), C.byref(self.desc), C.byref(self.res),
                                              self.matches.ctypes.data, self.rn.ctypes.data)

    def run(self) -> dict:
        self.ctx.check(self.run_raw())
        res = self.res
        sm = res.summary.as_dict()
        frame = self.cur_frame if self.cur_frame is not None else capi.DeviceFrame(self.ctx, C.c_void_p(res.frame))
        return dict(frame=frame, T_run=np.array(list(res.T_run)).reshape(3, 4),
                    n_tracked=int(res.n_tracked), lost=bool(res.lost), stats=res.stats.as_dict(), n_in_grid=int(res.n_in_grid),
                    replay_full_scan=bool(res.replay_full_scan), matches=self.matches[:res.n_matches].copy(),
                    T_opt=np.array(list(res.T_opt)).reshape(3, 4), summary=sm, residual_norm=self.rn[:sm["n_residual_blocks"]].copy())


def track_frame(ctx: capi.Context, cam, image, levels, last: Frame, T_seed, align, min_tracked, keyframes, map_points, **kw):
    """dsdtm_track_frame. `last` and the keyframes are Frames whose pyramids are (made) resident on the device; `align` =
    (max_level, min_level, max_iters, min_fts). Returns a dict: frame (capi.DeviceFrame of the new image), T_run, n_tracked, lost,
    stats, n_in_grid, matches (structured array: cell, point, px, level), T_opt, summary, residual_norm."""
    return TrackCall(ctx, cam, image, levels, last, T_seed, align, min_tracked, keyframes, map_points, **kw).run()


class TrackBatchCall:
    """One prepared dsdtm_track_frames call: n frames of n independent trackers (each described as for TrackCall: a dict of
    TrackCall's arguments), descriptors built once, `run()` the library call alone. Every frame's result equals its TrackCall's;
    each one also carries `in_grid` (uint8 per map point: 1 = ReprojectPoint put it into the grid, i.e. into mvpLocalMapPoints).
    With `cur_frames` (n capi.DeviceFrame from DeviceFrame.prefetch, .from_image or an earlier batch — or a `cur_frame` in every
    dict) the call runs in its resident mode: the new frames are already on the device, or on their way there, the images are not
    read, the chain starts at Run, and result f's "frame" is cur_frames[f] — still the caller's."""

    def __init__(self, ctx: capi.Context, cam, frames, cur_frames=None):
        self.ctx = ctx
        if cur_frames is not None:
            if len(cur_frames) != len(frames):
                raise ValueError(f"{len(cur_frames)} resident frames for {len(frames)} frames")
            frames = [dict(f, cur_frame=c) for f, c in zip(frames, cur_frames)]
        self.calls = [TrackCall(ctx, cam, **f) for f in frames]
        n = len(self.calls)
        self.n = n
        self.cur_frames = [c.cur_frame for c in self.calls]
        # (all or none; a mixture goes down as it is and the library names the first frame that differs)
        self.resident = n > 0 and all(c is not None for c in self.cur_frames)
        self.descs = (capi.TrackDesc * max(1, n))(*[c.desc for c in self.calls])
        self.res = (capi.TrackResult * max(1, n))()
        self.max_matches = int(self.calls[0].desc.max_matches) if n else 1
        self.matches = np.zeros(max(1, n * self.max_matches), capi.TRACK_MATCH_DTYPE)
        self.rn = np.zeros(max(1, n * self.max_matches))
        self.n_points = [int(c.desc.n_points) for c in self.calls]
        self.grid_at = np.concatenate([[0], np.cumsum(self.n_points)]).astype(np.int64)
        self.in_grid = np.zeros(max(1, int(self.grid_at[-1])), np.uint8)
        self.cs = capi.camera_struct(cam)

    def run_raw(self) -> int:
        """The library call alone; returns its status (the new frames' handles are in self.res[f].frame)."""
        if not self.resident:
            for f, c in enumerate(self.cur_frames):               # (a mixture: the resident ones are named, the library refuses)
                self.res[f].frame = c.handle.value if c is not None else None
        return capi.track_frames(self.ctx, self.cs, self.n, self.descs, self.res, self.matches.ctypes.data, self.rn.ctypes.data,
                                 self.in_grid.ctypes.data, frames=self.cur_frames if self.resident else None)

    def run(self) -> list:
        self.ctx.check(self.run_raw())
        out = []
        for f in range(self.n):
            res = self.res[f]
            sm = res.summary.as_dict()
            m0 = f * self.max_matches
            frame = self.cur_frames[f] if self.resident else capi.DeviceFrame(self.ctx, C.c_void_p(res.frame))
            out.append(dict(frame=frame, T_run=np.array(list(res.T_run)).reshape(3, 4),
                            n_tracked=int(res.n_tracked), lost=bool(res.lost), stats=res.stats.as_dict(), n_in_grid=int(res.n_in_grid),
                            replay_full_scan=bool(res.replay_full_scan), matches=self.matches[m0:m0 + res.n_matches].copy(),
                            T_opt=np.array(list(res.T_opt)).reshape(3, 4), summary=sm,
                            residual_norm=self.rn[m0:m0 + sm["n_residual_blocks"]].copy(),
                            in_grid=self.in_grid[self.grid_at[f]:self.grid_at[f + 1]].copy()))
        return out


def track_frames(ctx: capi.Context, cam, frames, cur_frames=None) -> list:
    """dsdtm_track_frames: `frames` is a list of dicts of track_frame's arguments after `cam` (image, levels, last, T_seed, align,
    min_tracked, keyframes, map_points, and its keywords). Returns one track_frame result per frame, plus `in_grid`.
    cur_frames=[capi.DeviceFrame, ...]: the resident mode (see TrackBatchCall) — `image` may then be None in every dict."""
    if not frames:
        return []
    return TrackBatchCall(ctx, cam, frames, cur_frames).run()


def apply_tracked_frame(cam, image, r, map_points, img_mask=None):
    """The reference's side effects of one tracked frame (src/Tracking.cpp:199-256) from a track_frame / track_frames result:
    returns (cur Frame, n_tracked, matches as [(cell, MapPoint, px float32[2], level)])."""
    cur = Frame(cam, [np.ascontiguousarray(image, np.uint8)], r["T_run"])              # (level 0 only on the host: the pyramid is on the device)
    cur._device_frame = r["frame"]
    if r["lost"]:                                                                      # :208-214
        return cur, r["n_tracked"], []
    m = r["matches"]
    mps = [map_points[int(i)] for i in m["point"]]
    for mp in mps:
        mp.IncreaseFound()                                                             # src/Feature_alignment.cpp:106
    if img_mask is not None:
        for q in m["px"]:                                                              # :111 (cv::Point from Point2d rounds)
            search.fill_circle(img_mask, search.cvRound(float(q[0])), search.cvRound(float(q[1])), int(Config.Get("Camera.CellSize")), 0)
    if len(m):
        search.add_matched_features(cur, m["px"], m["level"], mps)                     # :108-114
    cur.Set_Pose(r["T_opt"])                                                           # src/Optimizer.cpp:78
    thresh = float(np.float32(Config.Get("Optimization.LocalBAthreshhold"))) / float(np.float32(cam.f))
    rn = r["residual_norm"]
    for i in range(len(rn)):                                                           # :80-92 (every feature has a block here: index = block)
        if rn[i] > thresh and not mps[i].IsBad():
            mps[i].EraseFound()
    return cur, r["n_tracked"], [(int(m["cell"][k]), mps[k], m["px"][k].copy(), int(m["level"][k])) for k in range(len(m))]


def frame_map_points(frame) -> list:
    """The frame's map points in feature order, as NeedKeyframe and Get_SceneDepth walk them (`for it in mvFeatures: if
    (!(*it)->Mpt) continue`, src/Tracking.cpp:360-363, src/Frame.cpp:248-251): from reference-shaped features (objects with an
    `Mpt`), else from the mirror's mvMapPoints (one entry per feature, None where the feature has no map point)."""
    fts = getattr(frame, "mvFeatures", None)
    if fts is not None and all(hasattr(f, "Mpt") for f in fts):
        return [f.Mpt for f in fts if f.Mpt is not None]
    return [mp for mp in getattr(frame, "mvMapPoints", []) if mp is not None]


def keyframe_desc(cur, last_kf, local_keyframes) -> dict:
    """One tracker's inputs of dsdtm_need_keyframes (capi.KeyframeCall) from reference-shaped Frame / KeyFrame / MapPoint
    objects: both poses, Get_VaildMpNums() (src/Frame.cpp:330-340: the features that have a map point), the map points of the
    current frame and of the last keyframe in feature order with their IsBad(), the camera centres of mvpLocalKeyFrames."""
    def centre(kf):
        if hasattr(kf, "Get_CameraCnt"):
            return np.asarray(kf.Get_CameraCnt(), np.float64)
        T = np.asarray(kf.Get_Pose(), np.float64).reshape(3, 4)
        return -T[:, :3].T @ T[:, 3]
    mc, mk = frame_map_points(cur), frame_map_points(last_kf)
    return dict(T_cur_w=np.asarray(cur.Get_Pose(), np.float64).reshape(12), T_kf_w=np.asarray(last_kf.Get_Pose(), np.float64).reshape(12),
                n_valid=len(mc),
                cur_p_world=np.array([mp.Get_Pose() for mp in mc], np.float64).reshape(-1, 3),
                cur_bad=np.array([1 if mp.IsBad() else 0 for mp in mc], np.uint8),
                kf_p_world=np.array([mp.Get_Pose() for mp in mk], np.float64).reshape(-1, 3),
                kf_bad=np.array([1 if mp.IsBad() else 0 for mp in mk], np.uint8),
                local_kf_centre=np.array([centre(k) for k in local_keyframes], np.float64).reshape(-1, 3))


class Tracker:
    """Tracking's per-frame flow (src/Tracking.cpp:199-256) on top of track_frame, with the reference's side effects: the new
    Frame gets the pose, the features SearchLocalPoints creates (px, level, bearing, map point, mbInitial) and the refined
    pose; matched map points IncreaseFound (src/Feature_alignment.cpp:106); the mask gets its discs (:111); PoseOptimization's
    EraseFound walk runs on the block-ordered norms (src/Optimizer.cpp:80-92)."""

    def __init__(self, camera, ctx: capi.Context | None = None, max_level=None, min_level=None, max_iters=None, min_tracked=20, distortion=None):
        self.cam = camera
        self.ctx = ctx or capi.default_context()
        self.distortion = None if distortion is None else tuple(float(v) for v in distortion)          # k1 k2 p1 p2 k3 (src/Camera.cpp:62-67); None: rectified images
        self.levels = int(Config.Get("Camera.MaxPyraLevels") if max_level is None else max_level)       # src/Tracking.cpp:20-24
        self.min_level = int(Config.Get("Camera.MinPyraLevels") if min_level is None else min_level)
        self.max_iters = int(Config.Get("Optimization.MaxIter") if max_iters is None else max_iters)
        self.min_tracked = int(min_tracked)
        self.last_result = None
        self.last_frame = None         # the frame the last TrackFrame returned (CraeteKeyframe's default)
        self._prefetched = []          # [(image, capi.DeviceFrame)] in the order prefetch() was called

    def prefetch(self, image, depth=None, depth_scale: float = 5000.0):
        """Optional: sends a frame to the device ahead of its TrackFrame (dsdtm_frame_prefetch; returns at once). The capture
        loop calls it for frame k + 1 BEFORE TrackFrame of frame k, so that the upload and the pyramid of k + 1 run beside the
        tracking of k; TrackFrame(image, ...) with the same image object then starts at Run on that frame. With `depth` (uint16)
        the frame also carries the depth map, for DeviceFrame.lift. Returns the capi.DeviceFrame. At most two frames are kept
        (k and k + 1): a third prefetch releases the oldest one that TrackFrame never asked for."""
        df = capi.DeviceFrame.prefetch(self.ctx, image, self.levels, depth, depth_scale)
        self._prefetched.append((image, df))
        while len(self._prefetched) > 2:
            self._prefetched.pop(0)[1].close()
        return df

    def _undistort(self):
        """The undistort add-on's context and this camera's map (built once), where a distortion was given."""
        from . import undistort
        if self.distortion is None:
            raise ValueError("this Tracker was made without a distortion: its images are rectified already")
        if getattr(self, "_undistort_ctx", None) is None:
            self._undistort_ctx = undistort.UndistortContext(self.ctx.device if hasattr(self.ctx, "device") else 0)
            self._undistort_map = self._undistort_ctx.make_map(self.cam, self.distortion)
        return self._undistort_ctx, self._undistort_map

    def prefetch_raw(self, image, depth=None, depth_scale: float = 5000.0):
        """prefetch() for a RAW sensor frame (a Tracker made with `distortion`): cv::undistort, which the reference switched off for its
        cost (src/Frame.cpp:57-61), through dsdtm_undistort_frames into torch device tensors, then the existing prefetch on their
        data_ptr(). `image` (uint8) and `depth` (uint16 or None): 2-D numpy arrays or torch tensors. TrackFrame(image, ...) with the
        same image object starts at Run on the rectified frame, and the Frame it returns is marked `rectified`: CraeteKeyframe does
        not move its features a second time (prefetch_raw and UndistortFeatures are ALTERNATIVES: the image is rectified, or the
        features detected on a raw image are). The Frame object keeps the caller's RAW host image; the rectified one is the returned
        tensor. Returns (capi.DeviceFrame, rectified gray, rectified depth (int16 holding the uint16 bytes) or None); the tensors
        stay alive with the frame."""
        import torch
        uctx, umap = self._undistort()
        dev = torch.device("cuda", uctx.device)
        h, w = umap.height, umap.width
        gray_t = torch.empty((h, w), dtype=torch.uint8, device=dev)
        depth_t = torch.empty((h, w), dtype=torch.int16, device=dev) if depth is not None else None      # (int16: the bytes of uint16)
        torch.cuda.synchronize(dev)              # (the tensors exist; the add-on's stream is its own)
        uctx.undistort_frames([dict(map=umap, gray_src=image, gray_dst=gray_t, depth_src=depth, depth_dst=depth_t)])
        df = capi.DeviceFrame.prefetch(self.ctx, (gray_t.data_ptr(), w, h, gray_t.stride(0)), self.levels,
                                       None if depth_t is None else (depth_t.data_ptr(), depth_t.stride(0)), depth_scale)
        df._keep = [gray_t, depth_t]
        df.rectified = True
        self._prefetched.append((image, df))
        while len(self._prefetched) > 2:
            self._prefetched.pop(0)[1].close()
        return df, gray_t, depth_t

    def prefetch_equalized(self, image, depth=None, depth_scale: float = 5000.0):
        """prefetch() behind cv::createCLAHE(3.0, cv::Size(8, 8))->apply, what the reference's drivers do to every image before the
        detector (Test/test_Feature_detection.cpp:85-86): dsdtm_clahe_apply into a torch device tensor, then the existing prefetch on
        its data_ptr(). `image` (uint8): a 2-D numpy array or torch tensor; `depth` goes to prefetch() as it is. TrackFrame(image, ...)
        with the same image object starts at Run on the equalised frame. The Frame object keeps the caller's image; the equalised one
        is the returned tensor. Returns (capi.DeviceFrame, equalised gray); the tensor stays alive with the frame."""
        import torch
        from . import clahe
        if getattr(self, "_clahe_ctx", None) is None:
            self._clahe_ctx = clahe.ClaheContext(self.ctx.device if hasattr(self.ctx, "device") else 0)
        dev = torch.device("cuda", self._clahe_ctx.device)
        gray_t = torch.empty(tuple(image.shape), dtype=torch.uint8, device=dev)
        torch.cuda.synchronize(dev)              # (the tensor exists; the add-on's stream is its own)
        self._clahe_ctx.apply(image, gray_t)
        h, w = gray_t.shape
        df = capi.DeviceFrame.prefetch(self.ctx, (gray_t.data_ptr(), w, h, gray_t.stride(0)), self.levels, depth, depth_scale)
        df._keep = list(df._keep) + [gray_t]
        self._prefetched.append((image, df))
        while len(self._prefetched) > 2:
            self._prefetched.pop(0)[1].close()
        return df, gray_t

    def UndistortFeatures(self, frame):
        """Frame::UndistortFeatures (src/Frame.cpp:94-150) on `frame`: the pixel of every feature that is not mbInitial goes through
        cv::undistortPoints(.., K, D, noArray(), K) (rule U5 of include/dsdtm_amd_undistort.h) and its bearing is recomputed, through
        dsdtm_undistort_points. (The C++ adapter evaluates undistort_points_host for one tracker, which is faster there; that
        function has no Python binding, and numpy is slower than the device call: profiles/r22_undistort.txt.) Nothing happens
        without a distortion, on a frame without features, and on a frame that came through prefetch_raw (its image was rectified:
        its features lie on the rectified image already)."""
        if self.distortion is None or frame.n_features == 0 or getattr(frame, "rectified", False):
            return frame
        uctx, _ = self._undistort()
        px, _ = uctx.undistort_points(self.cam, self.distortion, frame.px, frame.initial, bearing_out=frame.bearing)
        frame.px[:] = px
        return frame

    def TrackFrame(self, image, last: Frame, keyframes, map_points, img_mask=None):
        """Returns (cur Frame, n_tracked, matches as [(cell, MapPoint, px float32[2], level)])."""
        cur_frame = None
        at = next((i for i, (im, _) in enumerate(self._prefetched) if im is image), None)
        if at is not None:                     # frames prefetched before it were skipped by the caller: released
            for _, stale in self._prefetched[:at]:
                stale.close()
            cur_frame = self._prefetched[at][1]
            del self._prefetched[:at + 1]
        r = track_frame(self.ctx, self.cam, image, self.levels, last, last.Get_Pose(),
                        (self.levels, self.min_level, self.max_iters, int(Config.Get("Camera.Min_fts"))), self.min_tracked,
                        keyframes, map_points, mask=img_mask, cur_frame=cur_frame)
        self.last_result = r
        out = apply_tracked_frame(self.cam, image, r, map_points, img_mask)
        if getattr(cur_frame, "rectified", False):          # (from prefetch_raw)
            out[0].rectified = True
        self.last_frame = out[0]
        return out

    def keyframe_params(self) -> KeyframeParams:
        """Tracking's thresholds of NeedKeyframe: KeyFrame.min_rot / min_trans (src/Tracking.cpp:26-27), the constants of :354-378."""
        return KeyframeParams(min_rot=float(Config.Get("KeyFrame.min_rot")), min_trans=float(Config.Get("KeyFrame.min_trans")))

    def NeedKeyframe(self, cur, last_kf, local_keyframes, params=None) -> dict:
        """Tracking::NeedKeyframe (src/Tracking.cpp:347-410) for the tracked frame `cur` against the last keyframe and
        mvpLocalKeyFrames, through dsdtm_need_keyframe. Returns the verdict as a dict (need, reason, rule_mask, ...: the fields of
        dsdtm_keyframe_verdict). Reads the objects only: TrackFrame's results are untouched."""
        return capi.need_keyframe(self.ctx, self.cam, params or self.keyframe_params(), keyframe_desc(cur, last_kf, local_keyframes))

    def _newkf(self):
        from . import keyframe_creation
        if getattr(self, "_newkf_ctx", None) is None:
            self._newkf_ctx = keyframe_creation.NewKeyframeContext(self.ctx.device if hasattr(self.ctx, "device") else 0)
        return keyframe_creation, self._newkf_ctx

    def CraeteKeyframe(self, store, depth, cur=None, depth_scale: float = 5000.0):
        """Tracking::CraeteKeyframe (src/Tracking.cpp:412-464) for the tracked frame `cur` (default: the frame the last TrackFrame
        returned) on `store` (a track_map.TrackMapStore; over a ba_window.MappingContext the new keyframe's covisibility list is
        answered too): Set_ExistingFeatures, dsdtm_detect_cells_frame, dsdtm_newkf_make, points_write + keyframe_add,
        UpdateConnection. `depth`: the frame's uint16 depth image. The new features and points are appended to `cur`. Returns the
        dict of keyframe_creation.create_keyframes. Measured in C++ (profiles/r20_newkf.txt): the step is 179 us for one
        tracker against 190 us for Feature_detector::detect + Frame::Lift; this Python adapter adds its own object work on top."""
        kc, nctx = self._newkf()
        cur = cur if cur is not None else self.last_frame
        if cur is None:
            raise ValueError("CraeteKeyframe: no frame was given and TrackFrame has not returned one yet")
        out = kc.create_keyframes(self.ctx, nctx, self.cam, [cur], [store], [depth], depth_scale)[0]
        if self.distortion is not None:          # src/Tracking.cpp:417 (here behind the lift, which the one device call includes)
            self.UndistortFeatures(cur)
        return out

    def CreateInitialMapRGBD(self, store, depth, init_frame, depth_scale: float = 5000.0):
        """Tracking::CreateInitialMapRGBD (src/Tracking.cpp:147-196): CraeteKeyframe's call on a frame without features, plus the
        test of :182 — fewer than 100 new map points: nothing is written and None is returned (the reference releases the map)."""
        kc, nctx = self._newkf()
        if init_frame.n_features:
            raise ValueError("the initial frame has features already")
        if self.distortion is not None:          # src/Tracking.cpp:149 (a frame without features: nothing to move)
            self.UndistortFeatures(init_frame)
        return kc.create_keyframes(self.ctx, nctx, self.cam, [init_frame], [store], [depth], depth_scale, min_points=100)[0]

    def UpdateLocalMap(self, store, T, n_local: int = 10):
        """The keyframe and point selection of Tracking::UpdateLocalMap (src/Tracking.cpp:258-297, GetCloseKeyFrames included) for
        the pose T on `store` (a local_map.LocalMapStore: the map on the device), through dsdtm_localmap_select. Returns
        (keyframes, map_points) as TrackFrame takes them: map_points in the order the reference hands them to ReprojectPoint;
        keyframes = every keyframe of the store in index order, because a map point's mObservations are keyed by that index and
        Get_ClosetObs walks all of them, local or not. mvpLocalKeyFrames (what NeedKeyframe takes) is kept in
        self.local_keyframes. Measured (profiles/r17_local_map.txt): the device select is 140-190 us whatever the map; below about
        170 keyframes the host evaluation (select_local_map_host, 0.9 us per keyframe) is the faster call for one pose, above it
        this one (5.8x at 1000 keyframes); MultiTracker.UpdateLocalMaps with 64 sequences or more wins from 100 keyframes on."""
        (self.local_keyframes, map_points), = _select_local_maps(self.cam, [store], [T], n_local)
        return list(store.keyframes), map_points

    def CommitTrackedFrame(self, store, r, point_list):
        """A tracked frame's effects on the RESIDENT map (IncreaseFound, the EraseFound walk, the SetBadFlag cascade: rules T1-T4 of
        include/dsdtm_amd_slam.h) through dsdtm_slam_track_commit: what apply_tracked_frame did to the objects, on `store` (a
        track_map.TrackMapStore over a slam.SlamContext), with no found_write / points_write / keyframe_write. `r`: the track_frame
        result (TrackFrame keeps it in self.last_result); `point_list`: the `point` list store.local() returned for this frame.
        Returns the entry's answer (n_erased, n_bad, bad_points, found_after, points). Measured (profiles/r21_aftertrack.txt): 25-44 us per
        call; track_commit_host is faster unless a point goes bad on a map of more than about 200 keyframes."""
        from . import slam
        return slam.commit_tracked_frames(store.ctx, self.cam, [store], [r], [point_list])[0]


def _select_local_maps(cam, stores, Ts, n_local):
    """[(mvpLocalKeyFrames, local map points)] for n stores of ONE local_map.LocalMapContext, in one dsdtm_localmap_select."""
    from . import local_map
    if not stores:
        return []
    if any(s.ctx is not stores[0].ctx for s in stores):
        raise ValueError("the stores of one call share one LocalMapContext")
    return local_map.update_local_maps(stores[0].ctx, cam, stores, Ts, n_local)


class MultiTracker:
    """Tracker.TrackFrame for n independent sequences at once (a multi-camera rig, offline re-tracking, many robots): one
    dsdtm_track_frames call per step, then the reference's side effects per sequence, as Tracker.TrackFrame applies them.
    All sequences share the camera and the tracking parameters. Each result also keeps the local map points ReprojectPoint
    put into the grid (`last_results[i]["local_map_points"]`: UpdateLocalMap's mvpLocalMapPoints, src/Tracking.cpp:299-304, empty
    for a lost frame) — the candidates of the caller's IsinFrustum -> IncreaseVisible() step."""

    def __init__(self, camera, ctx: capi.Context | None = None, max_level=None, min_level=None, max_iters=None, min_tracked=20):
        self.t = Tracker(camera, ctx, max_level, min_level, max_iters, min_tracked)
        self.cam, self.ctx = camera, self.t.ctx
        self.last_results = []
        self._prefetched = []          # [(images, [capi.DeviceFrame])] per step, in the order prefetch() was called

    def prefetch(self, images, depths=None, depth_scale: float = 5000.0):
        """Optional, the batch twin of Tracker.prefetch: sends one step's n images (and depth maps, uint16) to the device ahead of
        their TrackFrames — one dsdtm_frame_prefetch per sequence, each returns at once. The lockstep loop calls it for step
        k + 1 BEFORE TrackFrames of step k; TrackFrames with the same image objects then starts at Run on those frames, and
        last_results[i]["frame"] is sequence i's resident frame (with its depth map: .lift for a keyframe). Returns the
        capi.DeviceFrames. At most two steps are kept: a third prefetch releases the oldest one TrackFrames never asked for."""
        depths = depths if depths is not None else [None] * len(images)
        if len(depths) != len(images):
            raise ValueError(f"{len(depths)} depth maps for {len(images)} images")
        dfs = []
        try:
            for im, dp in zip(images, depths):
                dfs.append(capi.DeviceFrame.prefetch(self.ctx, im, self.t.levels, dp, depth_scale))
        except Exception:
            for df in dfs:
                df.close()
            raise
        self._prefetched.append((list(images), dfs))
        while len(self._prefetched) > 2:
            for df in self._prefetched.pop(0)[1]:
                df.close()
        return dfs

    def TrackFrames(self, images, lasts, keyframes, map_points, img_masks=None):
        """Lists of n (one per sequence). Returns [(cur Frame, n_tracked, matches)] as Tracker.TrackFrame does per sequence."""
        n = len(images)
        cur_frames = None
        at = next((i for i, (ims, _) in enumerate(self._prefetched)
                   if len(ims) == n and all(a is b for a, b in zip(ims, images))), None)
        if at is not None:                     # steps prefetched before it were skipped by the caller: released
            for _, stale in self._prefetched[:at]:
                for df in stale:
                    df.close()
            cur_frames = self._prefetched[at][1]
            del self._prefetched[:at + 1]
        img_masks = img_masks if img_masks is not None else [None] * n
        align = (self.t.levels, self.t.min_level, self.t.max_iters, int(Config.Get("Camera.Min_fts")))
        frames = [dict(image=images[i], levels=self.t.levels, last=lasts[i], T_seed=lasts[i].Get_Pose(), align=align,
                       min_tracked=self.t.min_tracked, keyframes=keyframes[i], map_points=map_points[i], mask=img_masks[i])
                  for i in range(n)]
        rs = track_frames(self.ctx, self.cam, frames, cur_frames)
        out = []
        for i, r in enumerate(rs):
            r["local_map_points"] = [map_points[i][j] for j in np.flatnonzero(r["in_grid"])]
            out.append(apply_tracked_frame(self.cam, images[i], r, map_points[i], img_masks[i]))
        self.last_results = rs
        return out

    def NeedKeyframes(self, curs, last_kfs, local_keyframes, params=None) -> list:
        """Tracker.NeedKeyframe for the n sequences of a step in ONE dsdtm_need_keyframes call (lists of n: the frames TrackFrames
        returned, each sequence's last keyframe and its mvpLocalKeyFrames). Returns n verdict dicts."""
        if not (len(curs) == len(last_kfs) == len(local_keyframes)):
            raise ValueError(f"{len(curs)} frames, {len(last_kfs)} last keyframes, {len(local_keyframes)} local keyframe lists")
        descs = [keyframe_desc(c, k, lk) for c, k, lk in zip(curs, last_kfs, local_keyframes)]
        return capi.need_keyframes(self.ctx, self.cam, params or self.t.keyframe_params(), descs)

    def CraeteKeyframes(self, curs, stores, depths, depth_scale: float = 5000.0) -> list:
        """Tracker.CraeteKeyframe for the sequences of a step that need a keyframe, with ONE dsdtm_newkf_make_batch (lists of equal
        length: the frames TrackFrames returned, each sequence's store and uint16 depth image; sequences that share a store are made
        one after the other, because their point numbers follow each other, with one dsdtm_newkf_make each). The image work in
        front is still ONE synchronous dsdtm_detect_cells_frame per sequence (dsdtm_detect_cells_batch_device is not used yet), so
        the batch entry's gain reaches this call only behind n detect calls. Returns one dict per sequence."""
        kc, nctx = self.t._newkf()
        return kc.create_keyframes(self.ctx, nctx, self.cam, list(curs), list(stores), list(depths), depth_scale)

    def UpdateLocalMaps(self, stores, Ts, n_local: int = 10):
        """Tracker.UpdateLocalMap for the n sequences of a step in ONE dsdtm_localmap_select (stores of one
        local_map.LocalMapContext; a rig's sequences may share a store). Returns (keyframes, map_points), each a list of n, as
        TrackFrames takes them; self.local_keyframes[i] is sequence i's mvpLocalKeyFrames."""
        picked = _select_local_maps(self.cam, list(stores), list(Ts), n_local)
        self.local_keyframes = [lk for lk, _ in picked]
        return [list(s.keyframes) for s in stores], [mps for _, mps in picked]

    def NeedKeyframesOnMap(self, stores, curs, last_kfs, local_keyframes, params=None) -> list:
        """NeedKeyframes on the RESIDENT map, in ONE dsdtm_slam_need_keyframes (stores of one slam.SlamContext): no position crosses the
        link — each frame's map points go up as the store's point indices (feature order), the last keyframe and mvpLocalKeyFrames as
        its keyframe indices; positions, bad flags, the keyframe's slots and the camera centres are read from the map. last_kfs[i] and
        local_keyframes[i] are keyframe objects of stores[i]. Returns n verdict dicts, as NeedKeyframes does."""
        if not (len(stores) == len(curs) == len(last_kfs) == len(local_keyframes)):
            raise ValueError(f"{len(stores)} stores, {len(curs)} frames, {len(last_kfs)} last keyframes, {len(local_keyframes)} local keyframe lists")
        if not stores:
            return []
        if any(s.ctx is not stores[0].ctx for s in stores):
            raise ValueError("the stores of one call share one SlamContext")
        trackers = []
        for s, cur, kf, lks in zip(stores, curs, last_kfs, local_keyframes):
            mc = frame_map_points(cur)
            trackers.append(dict(map=s.map, T_cur_w=np.asarray(cur.Get_Pose(), np.float64).reshape(12), n_valid=len(mc), cur_point=[s.point_index(mp) for mp in mc],
                                 kf=s.keyframe_index(kf), local_kf=[s.keyframe_index(k) for k in lks]))
        return stores[0].ctx.need_keyframes(self.cam, params or self.t.keyframe_params(), trackers)

    def CommitTrackedFrames(self, stores, point_lists, results=None) -> list:
        """Tracker.CommitTrackedFrame for the n sequences of a step in ONE dsdtm_slam_track_commit (stores of one slam.SlamContext;
        sequences that share a store are applied in list order, as the lockstep loop applies them). `results` defaults to
        self.last_results. Returns n answers."""
        from . import slam
        results = self.last_results if results is None else results
        if not (len(stores) == len(point_lists) == len(results)):
            raise ValueError(f"{len(stores)} stores, {len(point_lists)} point lists, {len(results)} results")
        if not stores:
            return []
        if any(s.ctx is not stores[0].ctx for s in stores):
            raise ValueError("the stores of one call share one SlamContext")
        return slam.commit_tracked_frames(stores[0].ctx, self.cam, list(stores), list(results), list(point_lists))
