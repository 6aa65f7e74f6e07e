"""The cases of tests/test_undistort_cpu.py and tests/test_undistort_gpu.py: the smallest shapes at which libdsdtm_amd_undistort.so can still go
wrong, their expected outputs by the restatement (dsdtm_amd/undistort_restatement.py; computed once per session and never modified) and
the binary form in which the stand-alone host driver (tests/undistort_host/driver.cpp) reads them and answers.

Images come from an integer hash of (x, y, seed), not from a random generator: the same bytes everywhere."""
import functools
import hashlib
import struct

import numpy as np

from dsdtm_amd import undistort_restatement as R

KINECT_CAM = (517.306408, 516.469215, 318.643040, 255.313989)          # Config/kinect.yaml (TUM fr1), fx fy cx cy
KINECT_DIST = (0.262383, -0.953104, -0.005358, 0.002628, 1.163314)     # k1 k2 p1 p2 k3
ZERO = (0.0, 0.0, 0.0, 0.0, 0.0)
# kinect_yaml is held by one hash of the restatement's output (gray, then depth) and 64 spot pixels, not by a committed image
KINECT_SHA256 = "ca5f9bce1bce69f818aa28ed199516c4caee8ee4f74a32a787c6331aec2fceaf"
KINECT_SPOTS_GRAY = [0, 0, 0, 0, 0, 0, 0, 0, 0, 182, 132, 200, 152, 107, 150, 0, 0, 78, 151, 70, 193, 69, 235, 0, 0, 154, 45, 157, 70, 128, 124, 0, 0, 122, 181, 49, 244, 190, 58, 0, 0, 176, 168, 162, 159, 196, 181, 0, 0, 90, 111, 196, 29, 129, 91, 0, 0, 0, 0, 0, 0, 0, 0, 0]
KINECT_SPOTS_DEPTH = [0, 0, 0, 0, 0, 0, 0, 0, 0, 931, 1987, 3378, 0, 1640, 1979, 0, 0, 952, 2218, 3722, 2469, 1869, 2653, 0, 0, 4140, 2638, 408, 3039, 3607, 3848, 0, 0, 2814, 3568, 1865, 4202, 2760, 0, 0, 0, 1205, 419, 1237, 2619, 1031, 2874, 0, 0, 2648, 1119, 1486, 4324, 3162, 2493, 0, 0, 0, 0, 0, 0, 0, 0, 0]


def _hash(h, w, seed):
    y, x = np.meshgrid(np.arange(h, dtype=np.uint64), np.arange(w, dtype=np.uint64), indexing="ij")
    v = (x * np.uint64(73856093)) ^ (y * np.uint64(19349663)) ^ np.uint64(seed * 83492791 + 12345)
    v = (v * np.uint64(2654435761)) & np.uint64(0xFFFFFFFF)
    v ^= v >> np.uint64(15)
    v = (v * np.uint64(2246822519)) & np.uint64(0xFFFFFFFF)
    return v ^ (v >> np.uint64(13))


def gray_image(h, w, seed, stride=None):
    """(h, w) uint8 view into a buffer whose rows lie `stride` bytes apart; the padding holds 0xEE."""
    stride = stride or w
    buf = np.full((h, stride), 0xEE, np.uint8)
    buf[:, :w] = (_hash(h, w, seed) >> np.uint64(8)).astype(np.uint8)
    return buf[:, :w]


def depth_image(h, w, seed, stride=None):
    """(h, w) uint16, 400..4495 with one pixel in 16 zero (a hole); the padding holds 0xEEEE."""
    stride = stride or w
    v = _hash(h, w, seed + 1000)
    buf = np.full((h, stride), 0xEEEE, np.uint16)
    buf[:, :w] = np.where((v & np.uint64(15)) == 0, 0, 400 + ((v >> np.uint64(4)) & np.uint64(4095))).astype(np.uint16)
    return buf[:, :w]


def small_cam(w, h, f_per_width=0.9375):
    """A camera whose field of view makes r2 reach about 0.45 in the corners of a small image."""
    f = float(w) * f_per_width
    return (f, f, (w - 1) / 2.0, (h - 1) / 2.0)


def _frame(name, w, h, cam, dist, seed, depth=True, gs=0, gd=0, zs=0, zd=0):
    """strides: 0 = the width; gs / gd in bytes, zs / zd in elements"""
    c = dict(name=name, w=w, h=h, cam=tuple(cam) + (w, h), dist=tuple(dist), gray=gray_image(h, w, seed, gs or w),
             depth=depth_image(h, w, seed, zs or w) if depth else None, gd=gd or w, zd=zd or w)
    return c


@functools.lru_cache(maxsize=None)
def frame_cases():
    cs = [_frame("identity", 40, 24, small_cam(40, 24), ZERO, 1)]
    cs += [_frame(f"tail_widths_{w}", w, 9, small_cam(w, 9), (0.2, 0.0, 0.01, -0.01, 0.0), 10 + w, gs=w + 3, gd=w + 5, zs=w + 1, zd=w + 7) for w in (37, 38, 39, 40)]
    # (this focal length puts map entries into the one-pixel corner zones: pixels with 3 taps outside exist, see test_undistort_cpu.py)
    cs.append(_frame("barrel_strong", 64, 48, small_cam(64, 48, 1.0375), (0.6, 0.0, 0.0, 0.0, 0.0), 2))
    cs.append(_frame("pincushion", 64, 48, small_cam(64, 48), (-0.4, 0.0, 0.0, 0.0, 0.0), 3))
    cs.append(_frame("tangential_only", 64, 48, small_cam(64, 48), (0.0, 0.0, 0.05, -0.03, 0.0), 4))
    cs.append(_frame("kinect_yaml", 640, 480, KINECT_CAM, KINECT_DIST, 5))
    cs.append(_frame("min_side", 8, 8, small_cam(8, 8), (0.3, -0.1, 0.02, 0.01, 0.05), 6))
    de = _frame("depth_edges", 48, 32, small_cam(48, 32), (0.35, 0.0, 0.02, -0.01, 0.0), 7)
    de["depth"][:, :] = 1000                      # a depth step, a 0 hole, a 65535 pixel
    de["depth"][:, 24:] = 3000
    de["depth"][10:14, 8:13] = 0
    de["depth"][20, 30] = 65535
    cs.append(de)
    cs.append(_frame("gray_only", 44, 20, small_cam(44, 20), (0.25, 0.0, 0.0, 0.0, 0.0), 8, depth=False))
    cs.append(_frame("depth_given", 44, 20, small_cam(44, 20), (0.25, 0.0, 0.0, 0.0, 0.0), 9))
    return tuple(cs)


def frame_case(name):
    return next(c for c in frame_cases() if c["name"] == name)


FRAME_NAMES = ["identity", "tail_widths_37", "tail_widths_38", "tail_widths_39", "tail_widths_40", "barrel_strong", "pincushion", "tangential_only",
               "kinect_yaml", "min_side", "depth_edges", "gray_only", "depth_given"]
BEARING_FILL = 7.0          # what bearing_out holds before a call: the rows of skipped pixels keep it


@functools.lru_cache(maxsize=None)
def point_cases():
    cam, W, H = KINECT_CAM + (640, 480), 640, 480
    gx, gy = np.meshgrid(np.linspace(20.0, W - 21.0, 7), np.linspace(20.0, H - 21.0, 5))
    grid = np.stack([gx.ravel(), gy.ravel()], axis=1).astype(np.float32)
    border = np.array([[0, 0], [W - 1, 0], [0, H - 1], [W - 1, H - 1], [-0.5, 100.25], [W + 30.0, H + 20.0], [-40.0, -25.0], [W / 2, -10.0],
                       [318.643040, 255.313989], [W - 1, H / 2]], np.float32)
    rest = ((_hash(1, 400, 77)[0] % np.uint64(W * 8)).astype(np.float64) / 8.0, (_hash(1, 400, 78)[0] % np.uint64(H * 8)).astype(np.float64) / 8.0)
    many = np.stack(rest, axis=1).astype(np.float32)                   # 400 pixels: more than one 256-thread block
    return (dict(name="pts_grid", cam=cam, dist=KINECT_DIST, px=grid, skip=None),
            dict(name="pts_skip", cam=cam, dist=KINECT_DIST, px=many, skip=(np.arange(400) % 2).astype(np.uint8)),
            dict(name="pts_border", cam=cam, dist=KINECT_DIST, px=border, skip=None),
            dict(name="pts_zero_dist", cam=cam, dist=ZERO, px=grid, skip=None))


POINT_NAMES = ["pts_grid", "pts_skip", "pts_border", "pts_zero_dist"]


def point_case(name):
    return next(c for c in point_cases() if c["name"] == name)


# ---- expected outputs: the restatement, once
@functools.lru_cache(maxsize=None)
def expected_frame(name):
    c = frame_case(name)
    m = R.undistort_map(c["cam"], c["dist"], c["w"], c["h"])
    g, z = R.undistort_frame(m, c["gray"], c["depth"])
    for a in (m, g) + ((z,) if z is not None else ()):
        a.setflags(write=False)
    return dict(map=m, gray=g, depth=z)


@functools.lru_cache(maxsize=None)
def expected_points(name):
    c = point_case(name)
    px, b = R.undistort_points(c["cam"], c["dist"], c["px"], c["skip"], bearing_out=np.full((len(c["px"]), 3), BEARING_FILL, np.float64))
    px.setflags(write=False); b.setflags(write=False)
    return dict(px=px, bearing=b)


def kinect_digest():
    e = expected_frame("kinect_yaml")
    return hashlib.sha256(e["gray"].tobytes() + e["depth"].tobytes()).hexdigest()


def kinect_spots():
    """64 pixels spread over the image (an 8 x 8 lattice that reaches all four borders): (gray values, depth values)"""
    e = expected_frame("kinect_yaml")
    ys, xs = np.meshgrid(np.linspace(0, 479, 8).astype(int), np.linspace(0, 639, 8).astype(int), indexing="ij")
    return e["gray"][ys, xs].ravel().tolist(), e["depth"][ys, xs].ravel().tolist()


# ---- the binary form for tests/undistort_host/driver.cpp
def pack():
    fc, pc = frame_cases(), point_cases()
    out = [struct.pack("<ii", len(fc), len(pc))]
    for c in fc:
        gs = c["gray"].base.shape[1] if c["gray"].base is not None else c["w"]
        zs = (c["depth"].base.shape[1] if c["depth"].base is not None else c["w"]) if c["depth"] is not None else 0
        out.append(struct.pack("<7i", c["w"], c["h"], 1 if c["depth"] is not None else 0, gs, c["gd"], zs, c["zd"]))
        out.append(np.asarray(c["cam"][:4] + c["dist"], np.float32).tobytes())
        out.append((c["gray"].base if c["gray"].base is not None else c["gray"]).tobytes())
        if c["depth"] is not None:
            out.append((c["depth"].base if c["depth"].base is not None else c["depth"]).tobytes())
    for c in pc:
        n = len(c["px"])
        out.append(struct.pack("<ii", n, 1 if c["skip"] is not None else 0))
        out.append(np.asarray(c["cam"][:4] + c["dist"], np.float32).tobytes())
        out.append(np.ascontiguousarray(c["px"], np.float32).tobytes())
        if c["skip"] is not None:
            out.append(c["skip"].tobytes())
    return b"".join(out)


def unpack(blob):
    """The driver's answers: per frame case the map, the WHOLE gray and depth destination buffers (prefilled with 0xA5, so the padding
    shows a write outside a row); per point case px_out and bearing_out (prefilled with BEARING_FILL)."""
    o, frames, points = 0, [], []
    for c in frame_cases():
        w, h = c["w"], c["h"]
        m = np.frombuffer(blob, np.int32, w * h * 2, o).reshape(h, w, 2); o += m.nbytes
        g = np.frombuffer(blob, np.uint8, h * c["gd"], o).reshape(h, c["gd"]); o += g.nbytes
        z = None
        if c["depth"] is not None:
            z = np.frombuffer(blob, np.uint16, h * c["zd"], o).reshape(h, c["zd"]); o += z.nbytes
        frames.append(dict(map=m, gray=g, depth=z))
    for c in point_cases():
        n = len(c["px"])
        px = np.frombuffer(blob, np.float32, 2 * n, o).reshape(n, 2); o += px.nbytes
        b = np.frombuffer(blob, np.float64, 3 * n, o).reshape(n, 3); o += b.nbytes
        points.append(dict(px=px, bearing=b))
    assert o == len(blob), (o, len(blob))
    return frames, points


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


# ---- deliberately WRONG variants of the restatement, for the non-vacuity check of tests/test_undistort_cpu.py
def truncating_round(v):
    """WRONG on purpose: truncation toward zero where U1 says cvRound."""
    v = np.asarray(v, np.float64)
    with np.errstate(invalid="ignore"):
        r = np.trunc(np.clip(np.where(np.isfinite(v), v, 0.0), -2147483648.0, 2147483647.0)).astype(np.int64)
    return np.where(np.isfinite(v), r, R.OUTSIDE).astype(np.int32)


def remap_gray_no_bias(m, src):
    """WRONG on purpose: U2 without its + 512."""
    return R.remap_gray(m, src, bias=0)
