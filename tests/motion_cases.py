"""The worlds the motion-mask tests share (tests/test_motion_cpu.py, tests/test_motion_gpu.py): image sequences with their
homographies, the restatement's trace over each (computed once, never modified), the C twin's loader, and the comparison rule.

A world is a dict(name, width, height, stride, images [steps x height x stride uint8], H [steps x 9]). Its trace (trace_of) is, per
step, the restatement's state BEFORE the step, the state after it, the mask, m_DistImg, the exp arguments and the stale cells.
"""
import ctypes as C
import os
import subprocess

import numpy as np

from dsdtm_amd import motion_restatement as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAX_EXCUSED_SHARE = 0.005          # of a world's pixels (the comparison rule of tests/test_motion_gpu.py)
WORLD_D_SEED = 5
BRIGHT = 149                       # against a texture of 100..104


def translation(tx, ty):
    return [1.0, 0.0, float(tx), 0.0, 1.0, float(ty), 0.0, 0.0, 1.0]


def _texture(rng, h, w, lo=100, hi=105):
    """Random texture in blocks of 2 px. Worlds A-C keep every contrast under 50 grey levels, object against background included
    (BRIGHT), so that no variance reaches VAR_MIN_NOISE_T (2500) and exp is only ever handed 0 — and over 43, so that the squared
    distance passes 2 * MIN_BG_VAR (1800) and the mask fires."""
    coarse = rng.integers(lo, hi, size=((h + 1) // 2, (w + 1) // 2))
    return np.kron(coarse, np.ones((2, 2), np.int64))[:h, :w].astype(np.uint8)


def _with_stride(frames, stride, rng):
    """steps x h x stride, the bytes beyond the width random (a median that reads them is caught)."""
    n, h, w = frames.shape
    out = rng.integers(0, 256, size=(n, h, stride)).astype(np.uint8)
    out[:, :, :w] = frames
    return out


def world_a():
    """64x48 (16x12 cells): a texture that shifts with the camera, and a bright 12x12 square that moves 3 px per step on its own.
    H is a translation by 6.0 px and then by 2.5 px, along x, along y and along both: with no motion along an axis that axis' offset
    (di or dj) is exactly 0 and the neighbour on it is not visited; 6.0 px gives offsets of half a cell, 2.5 px other weights."""
    rng = np.random.default_rng(101)
    w, h, steps = 64, 48, 6
    shifts = [(6.0, 0.0), (2.5, 0.0), (0.0, 6.0), (0.0, 2.5), (6.0, 2.5), (2.5, 6.0)]
    big = _texture(rng, h + 64, w + 64)
    frames, ox, oy = [], 32.0, 32.0
    for s in range(steps):
        ox, oy = ox - shifts[s][0], oy - shifts[s][1]
        f = big[int(round(oy)):int(round(oy)) + h, int(round(ox)):int(round(ox)) + w].copy()
        f[10 + 3 * s:22 + 3 * s, 8 + 3 * s:20 + 3 * s] = BRIGHT
        frames.append(f)
    return dict(name="A", width=w, height=h, stride=w, images=np.stack(frames), H=[translation(*t) for t in shifts])


def world_b():
    """64x48: H translates by 1.5 cells along x for two consecutive steps and then by -1.5: the last cell column has all four source
    cells off the model (sumW == 0) twice running — m_Mean_Temp there is what the step before left — then the first column."""
    rng = np.random.default_rng(202)
    w, h = 64, 48
    frames = np.stack([_texture(rng, h, w) for _ in range(5)])
    return dict(name="B", width=w, height=h, stride=w, images=frames,
                H=[translation(0, 0), translation(6, 0), translation(6, 0), translation(-6, 0), translation(-6, 0)])


def world_c():
    """70x50 in a buffer of stride 80: neither side a multiple of 4 (17x12 cells, 2 columns and 2 rows belong to no cell), random bytes
    beyond the width."""
    rng = np.random.default_rng(303)
    w, h = 70, 50
    frames = np.stack([_texture(rng, h, w) for _ in range(4)])
    frames[2:, 20:34, 30:50] = BRIGHT
    return dict(name="C", width=w, height=h, stride=80, images=_with_stride(frames, 80, rng),
                H=[translation(0, 0), translation(1.0, -0.5), translation(-3.25, 2.0), translation(0.75, 0.75)])


def world_d(seed=WORLD_D_SEED):
    """96x64: a high-contrast checkerboard of 8-px squares (with a little noise) that drifts, under a mild perspective H
    (h6, h7 ~ 1e-4): cells that straddle a square's edge gather means that differ by ~200, the interpolated variance passes
    VAR_MIN_NOISE_T and the exp branch runs."""
    rng = np.random.default_rng(seed)
    w, h, steps = 96, 64, 6
    yy, xx = np.mgrid[0:h, 0:w]
    frames, Hs = [], []
    for s in range(steps):
        board = (((xx + 3 * s) // 8 + (yy + 2 * s) // 8) % 2) * 200 + 25
        frames.append(np.clip(board + rng.integers(-12, 13, size=(h, w)), 0, 255).astype(np.uint8))
        Hs.append([1.0 + 0.002 * s, 0.003, 2.5 + 0.5 * s, -0.002, 1.001, 1.75, 1.0e-4, -1.2e-4, 1.0])
    return dict(name="D", width=w, height=h, stride=w, images=np.stack(frames), H=Hs)


def world_real():
    """640x480 out of the one real image tests/golden holds (fast_reference.npz["test1"], 752x480): three crops that slide by 2 px —
    views into the 752-wide buffer, so the stride is 752 — the last one with a bright block pasted in."""
    img = np.load(os.path.join(ROOT, "tests", "golden", "fast_reference.npz"))["test1"]
    assert img.shape == (480, 752) and img.dtype == np.uint8
    frames = np.stack([np.ascontiguousarray(img) for _ in range(3)])
    frames[2, 200:260, 300:380] = 255
    return dict(name="real", width=640, height=480, stride=752, images=frames, offsets=[56, 58, 60],
                H=[translation(0, 0), translation(-2.0, 0), translation(-2.0, 0)])


WORLDS = {"A": world_a, "B": world_b, "C": world_c, "D": world_d, "real": world_real}
_WORLDS, _TRACES = {}, {}


def world(name):
    if name not in _WORLDS:
        _WORLDS[name] = WORLDS[name]()
    return _WORLDS[name]


def image_of(wd, step):
    """The step's image as a height x width view (rows `stride` apart)."""
    off = wd.get("offsets", [0] * len(wd["H"]))[step]
    return wd["images"][step][:, off:off + wd["width"]]


def run_world(wd, model_class=R.ProbModel, round_fn=None):
    """The restatement over a world. Per step: before / after (12 x cells), mask, dist, exp_arg, stale, gray."""
    rs = R.MotionRestatement(wd["width"], wd["height"], model_class)
    trace = []
    for s in range(len(wd["H"])):
        before = rs.model.state.copy()
        out = rs.step(image_of(wd, s), wd["H"][s])
        trace.append(dict(before=before, after=rs.model.state.copy(), **out))
    return trace


def trace_of(name):
    if name not in _TRACES:
        _TRACES[name] = run_world(world(name))
    return _TRACES[name]


def exp_cells(step_trace):
    """Cells whose compensation handed exp a non-zero argument (either mode)."""
    return (step_trace["exp_arg"] != 0.0).any(axis=0)


def excusable_pixels(wd, step_trace):
    """Pixels whose mask may differ from the restatement's: in an exp-branch cell AND |dist - 2 var| < 1e-4 dist, var = m_Var_Temp[0]
    after pass 1 of update = row VAR_T of the state after the step."""
    mw, mh = wd["width"] // 4, wd["height"] // 4
    cell = np.zeros((wd["height"], wd["width"]), bool)
    cell[:4 * mh, :4 * mw] = np.kron(exp_cells(step_trace).reshape(mh, mw), np.ones((4, 4), bool))
    var = np.zeros((wd["height"], wd["width"]), np.float64)
    var[:4 * mh, :4 * mw] = np.kron(step_trace["after"][R.VAR_T].astype(np.float64).reshape(mh, mw), np.ones((4, 4)))
    dist = step_trace["dist"].astype(np.float64)
    return cell & (np.abs(dist - 2.0 * var) < 1e-4 * dist)


def ulp_distance(a, b):
    """Distance in units in the last place between two float32 arrays (their ordered integer images)."""
    def ordered(x):
        i = np.ascontiguousarray(x, np.float32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7FFFFFFF), i)
    return np.abs(ordered(a) - ordered(b))


def features(name, n=200, seed=77):
    """n feature positions for a world's LAST mask and the restatement's flags for them: the four corner pixels, coordinates at exact
    halves (cvRound goes to the even neighbour), and the rest spread over the box around the mask's set pixels, where rounding up or
    down decides."""
    wd, mask = world(name), trace_of(name)[-1]["mask"]
    w, h = wd["width"], wd["height"]
    rng = np.random.default_rng(seed)
    ys, xs = np.nonzero(mask == 255)
    assert len(xs), name
    x0, x1, y0, y1 = max(xs.min() - 3, 0), min(xs.max() + 3, w - 1), max(ys.min() - 3, 0), min(ys.max() + 3, h - 1)
    px = np.stack([rng.uniform(x0, x1, n), rng.uniform(y0, y1, n)], axis=1).astype(np.float32)
    px[:4] = [[0, 0], [w - 1, 0], [0, h - 1], [w - 1, h - 1]]
    px[4:8] = [[-0.5, -0.5], [w - 0.5 - 1, h - 0.5 - 1], [w - 1 + 0.25, 0.5], [0.5, h - 1 + 0.49]]      # still inside after rounding
    half = np.floor(px[8:n // 2]) + 0.5
    px[8:n // 2] = np.minimum(half, [w - 1.5, h - 1.5])
    return px, R.MotionRestatement.features_on_mask(mask, px)


# ---- the C twin (tests/motion_restatement.c), compiled into a scratch directory ----
_TWIN = {}


def c_twin(tmp_dir, opt="-O2"):
    key = (str(tmp_dir), opt)
    if key not in _TWIN:
        so = os.path.join(str(tmp_dir), "libmotion_restatement.so")
        subprocess.run([os.environ.get("CC", "cc"), opt, "-ffp-contract=off", "-std=c11", "-shared", "-fPIC", "-o", so,
                        os.path.join(ROOT, "tests", "motion_restatement.c"), "-lm"], check=True)
        lib = C.CDLL(so)
        vp, i = C.c_void_p, C.c_int
        lib.motion_median5.restype, lib.motion_median5.argtypes = None, [vp, i, i, i, vp]
        lib.motion_model_init.restype, lib.motion_model_init.argtypes = None, [vp, i, i]
        lib.motion_step.restype, lib.motion_step.argtypes = i, [vp, i, i, vp, i, vp, vp, i, vp, vp, vp]
        _TWIN[key] = lib
    return _TWIN[key]


def run_world_c(lib, wd):
    """The C twin over a world: the same trace (before, after, mask, dist, exp_arg, n_stale, gray)."""
    w, h = wd["width"], wd["height"]
    nc = (w // 4) * (h // 4)
    st = np.zeros((12, nc), np.float32)
    lib.motion_model_init(st.ctypes.data, w, h)
    trace = []
    for s in range(len(wd["H"])):
        img = image_of(wd, s)
        H = np.ascontiguousarray(wd["H"][s], np.float64)
        mask, gray = np.full((h, w), 0xA5, np.uint8), np.zeros((h, w), np.uint8)
        dist, arg = np.zeros((h, w), np.float32), np.zeros((2, nc), np.float64)
        before = st.copy()
        n_stale = lib.motion_step(st.ctypes.data, w, h, img.ctypes.data, img.strides[0], H.ctypes.data, mask.ctypes.data, w,
                                  gray.ctypes.data, dist.ctypes.data, arg.ctypes.data)
        trace.append(dict(before=before, after=st.copy(), mask=mask, dist=dist, exp_arg=arg, n_stale=n_stale, gray=gray))
    return trace
