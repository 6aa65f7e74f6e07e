"""numpy restatement of dsdtm_frame_lift: Frame::Get_FeatureDetph(cv::Point2f) followed by Frame::UnProject
(reference src/Frame.cpp:152-157, 201-224; Camera::Pixel2Camera(Point2f, d), src/Camera.cpp:173-178; Sophus SE3::inverse and
SE3 * point). The operation order is the reference's: the projection in float, widened to double, then R^T p + (-(R^T t)) in
double with each three-term sum evaluated left to right."""
import numpy as np

from dsdtm_amd import tum


def lift(depth_m: np.ndarray, cam, T_c2w, px_xy):
    """depth_m: (H, W) float32 metres (tum.depth_to_metres); T_c2w: [R|t] 3x4 world -> camera; px_xy: (n, 2) float32.
    Returns (depth[n] float32 with -1 where the pixel has none, p_world[n, 3] float64, zero where depth is -1)."""
    px = np.asarray(px_xy, np.float32).reshape(-1, 2)
    T = np.asarray(T_c2w, np.float64).reshape(3, 4)
    R, t = T[:, :3], T[:, 3]
    fx, fy, cx, cy = (np.float32(v) for v in (cam.fx, cam.fy, cam.cx, cam.cy))
    n = px.shape[0]
    d_out = np.full(n, -1.0, np.float32)
    p_out = np.zeros((n, 3), np.float64)
    for i in range(n):
        d = np.float32(tum.get_feature_depth(depth_m, px[i]))
        d_out[i] = d
        if d == np.float32(-1.0):
            continue
        x = np.float32(np.float32(d * np.float32(px[i, 0] - cx)) / fx)          # depth*(point.x - mcx)/mfx, in float
        y = np.float32(np.float32(d * np.float32(px[i, 1] - cy)) / fy)
        p = np.array([np.float64(x), np.float64(y), np.float64(d)])
        for c in range(3):
            rp = (R[0, c] * p[0] + R[1, c] * p[1]) + R[2, c] * p[2]                # (R^T p)[c]
            rt = (R[0, c] * t[0] + R[1, c] * t[1]) + R[2, c] * t[2]                # (R^T t)[c]
            p_out[i, c] = rp + (-rt)
    return d_out, p_out


def ulp_bound(p_cam_abs_max: float, t_abs_max: float, ulps: int = 4) -> float:
    """`ulps` units in the last place of max(|p_c|, |t|): the kernel may contract a*b + c into one rounding where numpy rounds
    twice, and every component is a sum of six products of magnitude <= that maximum (|R_ij| <= 1)."""
    return ulps * float(np.spacing(np.float64(max(p_cam_abs_max, t_abs_max))))
