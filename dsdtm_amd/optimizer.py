"""Optimizer — host mirror of DSDTM::Optimizer::PoseOptimization (include/Optimizer.h:29,
src/Optimizer.cpp:20-101; called by Tracking::TrackWithLocalMap right after SearchLocalPoints,
src/Tracking.cpp:236) over the C ABI. The solve — every residual/Jacobian evaluation, the
trust-region iterations, the final residual norms — is one library call (dsdtm_pose_optimization,
HIP, one wavefront); what is left here is the reference's bookkeeping on MapPoint objects (:80-92).

Optimizer::LocalBundleAdjustment (src/Optimizer.cpp:103-282, called by LocalMapping::Run for every new keyframe) the
same way: the solve and the outlier test are one call (dsdtm_local_ba, HIP, one workgroup), the set construction,
write-back and outlier bookkeeping stay here, on KeyFrame / MapPoint objects (dsdtm_amd.mapping has minimal ones).

There is no CPU path for the solve.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import capi
from .frame import Config, Frame


class Optimizer:
    last_summary = None

    @staticmethod
    def PoseOptimization(tCurFrame: Frame, tIterations: int = 100, ctx: capi.Context | None = None):
        """tIterations is accepted and ignored, as in the reference (max_num_iterations = 100, :72).

        Reads tCurFrame.bearing / level / initial and tCurFrame.mvMapPoints (one entry per feature: an
        object with Get_Pose / IsBad / EraseFound, or None); writes the pose (Set_Pose, :78) and calls
        EraseFound on the map points the reference would (:80-92). Returns the solver summary."""
        ctx = ctx or capi.default_context()
        n = tCurFrame.n_features if len(tCurFrame.bearing) else 0
        mpts = list(getattr(tCurFrame, "mvMapPoints", [None] * n))
        assert len(mpts) == n, "mvMapPoints must have one entry per feature"
        use = np.zeros(n, np.uint8)
        pw = np.zeros((n, 3), np.float64)
        tvMpts = {}                                              # feature index -> MapPoint (:43, :57)
        for i in range(n):                                       # :45-65
            mp = mpts[i]
            if mp is None or mp.IsBad() or not tCurFrame.initial[i]:
                continue
            use[i] = 1
            pw[i] = mp.Get_Pose()
            tvMpts[i] = mp
        T = np.ascontiguousarray(tCurFrame.Get_Pose(), np.float64).reshape(12).copy()
        rn, sm = pose_optimization(ctx, tCurFrame.bearing, pw, tCurFrame.level, use, T)
        tCurFrame.Set_Pose(T.reshape(3, 4))                      # :78
        # :22-24: double(float threshold) / float mf
        thresh = float(np.float32(Config.Get("Optimization.LocalBAthreshhold"))) / float(np.float32(tCurFrame.mCamera.f))
        # :80-92 — the residual vector is in residual-BLOCK order while tvMpts is keyed by FEATURE index
        # (std::map::operator[] yields NULL for a missing key); the reference mixes the two and so do we
        for i in range(len(rn)):
            if rn[i] > thresh:
                mp = tvMpts.get(i)
                if mp is None:
                    continue
                if mp.IsBad():
                    continue
                mp.EraseFound()
        Optimizer.last_summary = sm
        return sm

    @staticmethod
    def LocalBundleAdjustment(tKFrame, tMap=None, ctx: capi.Context | None = None, solve=None):
        """src/Optimizer.cpp:103-282 on duck-typed keyframes (mlId, mlLocalBAKfId, mlFixedLocalBAKfId, mvMapPoints,
        mvFeatures[i].mNormal / .mlevel, mCamera.mf, Get_Pose / Set_Pose, GetCovKFrames, Erase_MapPointMatch) and map
        points (mlID, mlLocalBAKFId, IsBad, Get_Pose / Set_Pose, Get_Observations, Erase_Observation). tMap is only
        the reference's lock holder. `solve` replaces the library call (tests of the bookkeeping); it takes and returns
        what local_bundle_adjustment does. Returns the solver summary (+ "n_outliers")."""
        cam = tKFrame.mCamera                                    # :105-106: double(float threshold) / float mf
        mf = cam.mf if hasattr(cam, "mf") else cam.f
        thresh = float(np.float32(Config.Get("Optimization.LocalBAthreshhold"))) / float(np.float32(mf))
        local_kfs = [tKFrame]                                    # :110-121
        for _, kf in tKFrame.GetCovKFrames():
            kf.mlLocalBAKfId = tKFrame.mlId
            local_kfs.append(kf)
        local_mps = []                                           # :123-141
        for kf in local_kfs:
            for mp in list(kf.mvMapPoints):
                if mp is None or mp.IsBad():
                    continue
                if mp.mlLocalBAKFId != tKFrame.mlId:
                    mp.mlLocalBAKFId = tKFrame.mlId
                    local_mps.append(mp)
        fixed_kfs = []                                           # :143-159
        for mp in local_mps:
            for kf in mp.Get_Observations():
                if kf.mlLocalBAKfId != tKFrame.mlId and kf.mlFixedLocalBAKfId != tKFrame.mlId:
                    kf.mlFixedLocalBAKfId = tKFrame.mlId
                    fixed_kfs.append(kf)
        # parameter blocks (:166-200): keyed by mlId as tKFPoseSets is, local keyframes first
        kf_index, kfs, const = {}, [], []
        for kf, fixed in [(k, False) for k in local_kfs] + [(k, True) for k in fixed_kfs]:
            if kf.mlId in kf_index:
                if fixed:
                    const[kf_index[kf.mlId]] = True              # SetParameterBlockConstant on the same block
                continue
            kf_index[kf.mlId] = len(kfs)
            kfs.append(kf)
            const.append(fixed or kf.mlId == 0)
        # residual blocks (:202-224): points in tvLocalMapPoints order, then their observations in map order
        obs_kf, obs_pt, bearing, level, pairs = [], [], [], [], []
        for q, mp in enumerate(local_mps):
            for kf, idx in mp.Get_Observations().items():
                if kf.mlId not in kf_index:
                    continue
                ft = kf.mvFeatures[idx]
                obs_kf.append(kf_index[kf.mlId]); obs_pt.append(q)
                bearing.append(np.asarray(ft.mNormal, np.float64)); level.append(int(ft.mlevel))
                pairs.append((mp, kf))
        T = np.stack([np.asarray(kf.Get_Pose(), np.float64).reshape(3, 4) for kf in kfs]).reshape(-1).copy()
        X = np.stack([np.asarray(mp.Get_Pose(), np.float64).reshape(3) for mp in local_mps]).reshape(-1).copy() \
            if local_mps else np.zeros(0)
        args = (T, np.asarray(const, np.uint8), X, np.asarray(obs_kf, np.int32), np.asarray(obs_pt, np.int32),
                np.asarray(bearing, np.float64).reshape(-1, 3), np.asarray(level, np.int32), thresh)
        if solve is None:
            out, sm = local_bundle_adjustment(ctx or capi.default_context(), *args)
        else:
            out, sm = solve(*args)
        for k, kf in enumerate(kfs):                             # :236-242 (every keyframe, fixed ones included)
            kf.Set_Pose(T.reshape(-1, 3, 4)[k].copy())
        for q, mp in enumerate(local_mps):                       # :244-248
            mp.Set_Pose(X.reshape(-1, 3)[q].copy())
        # :250-271 — Erase_Observation runs first, so Erase_MapPointMatch finds no index (Get_IndexInKeyFrame == -1) and
        # the keyframe's mvMapPoints entry stays; Erase_Observation sets a point left with <= 1 observation bad
        for i in np.nonzero(out)[0]:
            mp, kf = pairs[i]
            mp.Erase_Observation(kf)
            kf.Erase_MapPointMatch(mp)
        Optimizer.last_summary = sm
        return sm

    @staticmethod
    def LocalBundleAdjustmentOnDevice(mctx, dmap, kf: int, cov_kf, origin_kf: int = -1, delta: float | None = None, ctx: capi.Context | None = None,
                                      capacities=(capi.LBA_MAX_FREE_KF + capi.LBA_MAX_CONST_KF, capi.LBA_MAX_POINTS, capi.LBA_MAX_OBSERVATIONS),
                                      max_iterations: int = 10, bad_capacity: int = 256, mf: float = 1.0):
        """src/Optimizer.cpp:103-282 on a map that is resident on the device (include/dsdtm_amd_mapping.h): window ->
        dsdtm_local_ba_batch_device -> commit, with no column crossing the link. mctx: a ba_window.MappingContext; dmap: its map;
        kf, cov_kf, origin_kf: map indices (cov_kf = the keyframe's stored GetCovKFrames(), normally what dsdtm_mapping_covisibility
        returned when it was created). delta None: double(float Optimization.LocalBAthreshhold) / float mf (:105-106).
        Returns None when the window is not usable — the caller takes LocalBundleAdjustment above, the host path, for that keyframe —
        else a dict: window (counts, flags, kf_index / point_index / obs_slot for the bookkeeping on the host's objects), outlier
        (the solver's flags per observation), summary, commit (n_outliers, n_bad, overflow_bad, bad_points: map indices)."""
        import torch
        from . import ba_window
        if delta is None:
            delta = float(np.float32(Config.Get("Optimization.LocalBAthreshhold"))) / float(np.float32(mf))
        ctx = ctx or capi.default_context()
        call = ba_window.WindowCall(mctx, [(dmap, kf, cov_kf, origin_kf, *capacities)])
        win = call.run()[0]
        if not win["usable"]:
            return None
        t = call.tensors
        outlier = torch.zeros(max(call.total["obs"], 1), dtype=torch.uint8, device=t["T_c2w"].device)
        summary = torch.zeros(capi.LBA_SUMMARY_DTYPE.itemsize, dtype=torch.uint8, device=t["T_c2w"].device)
        prm = capi.LocalBaParams(int(max_iterations), 0, float(delta))
        # (a prototype of its own: the library handle's shared function object is left as other callers set it)
        proto = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int, C.c_void_p, *([C.c_void_p] * 7), C.POINTER(capi.LocalBaParams), C.c_void_p, C.c_void_p, C.c_void_p)
        f = proto(("dsdtm_local_ba_batch_device", ctx.lib))
        stream = torch.cuda.current_stream()
        ctx.check(f(ctx.handle, 1, C.cast(call.problems, C.c_void_p), t["T_c2w"].data_ptr(), t["kf_constant"].data_ptr(), t["points"].data_ptr(),
                    t["obs_kf"].data_ptr(), t["obs_point"].data_ptr(), t["obs_bearing"].data_ptr(), t["obs_level"].data_ptr(), C.byref(prm),
                    outlier.data_ptr(), summary.data_ptr(), C.c_void_p(stream.cuda_stream)))
        # (no wait here: the commit orders itself behind the solve on the device)
        st, res = call.commit(outlier, C.c_void_p(stream.cuda_stream), bad_capacity)
        mctx.check(st)
        sm = np.frombuffer(summary.cpu().numpy().tobytes(), capi.LBA_SUMMARY_DTYPE)[0]
        nk, npt = win["n_local"] + win["n_fixed"], win["n_points"]
        out = dict(window=win, outlier=outlier[:win["n_obs"]].cpu().numpy(), summary={k: sm[k].item() for k in sm.dtype.names}, commit=res[0],
                   T_c2w=call.column("T_c2w")[:nk].copy(), points=call.column("points")[:npt].copy())
        Optimizer.last_summary = out["summary"]
        return out


def pose_optimization(ctx: capi.Context, bearing, p_world, level, use, T_cur_w, max_iterations: int = 100):
    """dsdtm_pose_optimization: T_cur_w (12 doubles) is updated in place; returns (residual norms in
    residual-block order, summary dict)."""
    bearing = np.ascontiguousarray(bearing, np.float64).reshape(-1, 3)
    pw = np.ascontiguousarray(p_world, np.float64).reshape(-1, 3)
    level = np.ascontiguousarray(level, np.int32)
    use = np.ascontiguousarray(use, np.uint8)
    n = len(use)
    assert len(bearing) == n and len(pw) == n and len(level) == n
    assert T_cur_w.dtype == np.float64 and T_cur_w.size == 12 and T_cur_w.flags.c_contiguous
    rn = np.zeros(max(n, 1))
    prm = capi.PoseOptParams(int(max_iterations), 0)
    sm = capi.PoseOptSummary()
    dp = C.POINTER(C.c_double)
    f = ctx.lib.dsdtm_pose_optimization
    f.restype = C.c_int
    f.argtypes = [C.c_void_p, dp, dp, C.POINTER(C.c_int32), capi.u8p, C.c_int, dp, C.POINTER(capi.PoseOptParams), dp,
                  C.POINTER(capi.PoseOptSummary)]
    ctx.check(f(ctx.handle, bearing.ctypes.data_as(dp), pw.ctypes.data_as(dp), level.ctypes.data_as(C.POINTER(C.c_int32)),
                use.ctypes.data_as(capi.u8p), n, T_cur_w.ctypes.data_as(dp), C.byref(prm), rn.ctypes.data_as(dp),
                C.byref(sm)))
    d = sm.as_dict()
    return rn[:d["n_residual_blocks"]].copy(), d


def local_bundle_adjustment(ctx: capi.Context, T_c2w, kf_constant, points, obs_kf, obs_point, obs_bearing, obs_level,
                            delta: float, max_iterations: int = 10):
    """dsdtm_local_ba: T_c2w (12 doubles per keyframe) and points (3 per point) are float64 C-contiguous arrays updated in
    place; returns (outlier flags per observation, summary dict)."""
    for a in (T_c2w, points):
        assert a.dtype == np.float64 and a.flags.c_contiguous and a.flags.writeable
    K, NP = T_c2w.size // 12, points.size // 3
    kc = np.ascontiguousarray(kf_constant, np.uint8)
    okf = np.ascontiguousarray(obs_kf, np.int32)
    opt = np.ascontiguousarray(obs_point, np.int32)
    b = np.ascontiguousarray(obs_bearing, np.float64).reshape(-1, 3)
    lev = np.ascontiguousarray(obs_level, np.int32)
    N = len(okf)
    assert len(kc) == K and len(opt) == N and len(b) == N and len(lev) == N
    out = np.zeros(max(N, 1), np.uint8)
    prm = capi.LocalBaParams(int(max_iterations), 0, float(delta))
    sm = capi.LocalBaSummary()
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    f = ctx.lib.dsdtm_local_ba
    f.restype = C.c_int
    f.argtypes = [C.c_void_p, C.c_int, dp, capi.u8p, C.c_int, dp, C.c_int, ip, ip, dp, ip, C.POINTER(capi.LocalBaParams),
                  capi.u8p, C.POINTER(capi.LocalBaSummary)]
    ctx.check(f(ctx.handle, K, T_c2w.ctypes.data_as(dp), kc.ctypes.data_as(capi.u8p), NP, points.ctypes.data_as(dp), N,
                okf.ctypes.data_as(ip), opt.ctypes.data_as(ip), b.ctypes.data_as(dp), lev.ctypes.data_as(ip), C.byref(prm),
                out.ctypes.data_as(capi.u8p), C.byref(sm)))
    return out[:N].copy(), sm.as_dict()
