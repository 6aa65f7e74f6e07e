"""The moving-object mask of fastMCD restated in numpy — the yardstick dsdtm_motion_step (csrc/motion.hip) is held to.
No device, no library call.

What it restates: MCDWrapper::Run (Thirdparty/fastMCD/src/MCDWrapper.cpp:65-137) up to and including BGModel.update(detect_img):
the 5x5 median of the image (cvSmooth(CV_MEDIAN, 5): the median of 25 bytes, BORDER_REPLICATE), then ProbModel::motionCompensate
and ProbModel::update (Thirdparty/fastMCD/include/prob_model.h:169-371, :373-582) on a model of floor(w/4) x floor(h/4) cells;
and the test of Frame::Motion_Removal (src/Frame.cpp:352) against that mask. Not restated: findHomography, the contour step
(MCDWrapper.cpp:98-128), KLTWrapper, Mod_FrameDiff.

Every cell of a step depends on the OLD m_Mean / m_Var / m_Age of up to four cells and on its own _Temp entries only, so a step is
written once for an array of cells (`_cells`) and run over all of them against a copy of the old model.

Types are the reference's as compiled with -std=c++11: every variable and array element is float32; a right-hand side in which a
double literal or h[] takes part is evaluated in float64 and rounded once where it is assigned; pow(float, (int)2) is the exact
float64 product of the float32 difference; the comparisons against 2.0 * var are float64; exp is libm's double exp (math.exp, so
that the C twin tests/motion_restatement.c agrees to the bit — numpy's vector exp is another implementation).
OpenCV's MAX(a, b) is (a < b ? b : a), MIN(a, b) is (a > b ? b : a).

The reference's ProbModel::init runs on a cvCreateImage buffer nobody has written yet and leaves the _Temp arrays of `new float[]`
unset; zeros are this project's definition of both.
"""
from __future__ import annotations

import math

import numpy as np

f32, f64 = np.float32, np.float64
MEAN, VAR, AGE, MEAN_T, VAR_T, AGE_T = 0, 2, 4, 6, 8, 10       # rows of the state (mode 0, then mode 1)
ARRAYS = ("m_Mean", "m_Var", "m_Age", "m_Mean_Temp", "m_Var_Temp", "m_Age_Temp")
BLOCK = 4
MAX_BG_AGE, VAR_MIN_NOISE_T, VAR_DEC_RATIO, MIN_BG_VAR, INIT_BG_VAR = 2.0, 50.0 * 50.0, 0.001, 30.0 * 30.0, 15.0 * 15.0
INDEX_LIMIT = 2.0 ** 30          # a transformed cell index of this magnitude or more is off the model (header: dsdtm_motion_step)
IDENTITY = (1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0)


def median5(image) -> np.ndarray:
    """The median of the 25 bytes around each pixel, the border replicated."""
    img = np.asarray(image, np.uint8)
    h, w = img.shape
    pad = np.pad(img, 2, mode="edge")
    taps = np.stack([pad[dy:dy + h, dx:dx + w] for dy in range(5) for dx in range(5)])
    return np.sort(taps, axis=0)[12]


def _max(a, b):
    return np.where(a < b, b, a)


def _min(a, b):
    return np.where(a > b, b, a)


def _exp(arg):
    out = np.ones(arg.shape, f64)
    for k in np.flatnonzero(arg.reshape(-1) != 0.0):
        out.reshape(-1)[k] = math.exp(float(arg.reshape(-1)[k]))
    return out


class ProbModel:
    """One ProbModel: `state` is the twelve arrays (12, cells) float32 in the order of ARRAYS x mode."""

    def __init__(self, width: int, height: int):
        self.w, self.h = int(width), int(height)
        self.mw, self.mh = self.w // BLOCK, self.h // BLOCK
        self.nc = self.mw * self.mh
        self.state = np.zeros((12, self.nc), f32)
        self.init()

    def init(self):
        """ProbModel::init (:121-167): zeros, then motionCompensate(identity) + update(NULL) on an all-zero image."""
        self.state[:] = 0
        self.model_step(None, IDENTITY, want_mask=False)

    # ---- the places a careless restatement (or kernel) goes wrong; tests/test_motion_cpu.py overrides one at a time ----
    def begin_step(self):
        """The _Temp arrays persist across steps: nothing is cleared."""

    def square(self, d):
        """pow(d, (int)2) of a float32 d: the exact float64 product."""
        return d.astype(f64) * d.astype(f64)

    def on_border(self, iI, iJ):
        """:357"""
        return (iI < 1) | (iI >= self.mw - 1) | (iJ < 1) | (iJ >= self.mh - 1)

    def mode1_is_oldest(self, age1, old_age):
        """:425: >= against the age so far, so equal ages pick mode 1."""
        return age1 >= old_age

    def oldest_to_front(self, pick, t, cur_mean):
        """:430-439: mode 0 receives mode 1; mode 1 becomes (cur_mean, INIT_BG_VAR, 0). Not a swap."""
        for arr, fresh in ((MEAN_T, cur_mean), (VAR_T, f32(INIT_BG_VAR)), (AGE_T, f32(0))):
            t[arr] = np.where(pick, t[arr + 1], t[arr])
            t[arr + 1] = np.where(pick, fresh, t[arr + 1]).astype(f32)

    def mask_variance(self, var_temp0, var_new0):
        """:546 uses m_Var_Temp[0], the variance from BEFORE this step's update."""
        return var_temp0

    def run_cells(self, px, H, out):
        """All cells against the model as it was before this step (update overwrites what compensation reads)."""
        self._cells(np.arange(self.nc), self.state[:6].copy(), px, H, out)

    # ---- one step ----
    def model_step(self, gray, H, want_mask=True):
        """motionCompensate(H) + update(out) on an already median-filtered image (None: all zeros). Returns a dict: mask (h x w uint8,
        255 / 0, None for update(NULL)), dist (m_DistImg), exp_arg (2 x cells: what exp was handed, 0 where it is not reached),
        stale (the cells with sumW == 0), mean_gray."""
        H = [float(v) for v in np.asarray(H, f64).reshape(9)]
        gray = np.zeros((self.h, self.w), np.uint8) if gray is None else np.asarray(gray, np.uint8)
        assert gray.shape == (self.h, self.w)
        px = gray[:self.mh * BLOCK, :self.mw * BLOCK].reshape(self.mh, BLOCK, self.mw, BLOCK).transpose(0, 2, 1, 3).reshape(self.nc, 16)
        out = dict(mask=np.zeros((self.h, self.w), np.uint8) if want_mask else None, dist=np.zeros((self.h, self.w), f32),
                   exp_arg=np.zeros((2, self.nc), f64), stale=np.zeros(self.nc, bool))
        self.begin_step()
        with np.errstate(all="ignore"):
            self.run_cells(px, H, out)
        return out

    def _cells(self, idx, src, px, H, out):
        mw, mh, st = self.mw, self.mh, self.state
        px = px[idx]
        i, j = idx % mw, idx // mw
        # ---- motionCompensate (:183-367) ----
        X, Y = (BLOCK * i + BLOCK / 2.0).astype(f32).astype(f64), (BLOCK * j + BLOCK / 2.0).astype(f32).astype(f64)
        newW = (H[6] * X + H[7] * Y + H[8]).astype(f32).astype(f64)
        newX = ((H[0] * X + H[1] * Y + H[2]) / newW).astype(f32)
        newY = ((H[3] * X + H[4] * Y + H[5]) / newW).astype(f32)
        newI, newJ = (newX.astype(f64) / 4.0).astype(f32), (newY.astype(f64) / 4.0).astype(f32)
        fI, fJ = np.floor(newI), np.floor(newJ)
        okI, okJ = np.abs(fI) < INDEX_LIMIT, np.abs(fJ) < INDEX_LIMIT
        iI, iJ = np.where(okI, fI, -2).astype(np.int64), np.where(okJ, fJ, -2).astype(np.int64)
        di = np.where(okI, (newI.astype(f64) - (iI.astype(f32).astype(f64) + 0.5)).astype(f32), f32(0.5)).astype(f32)
        dj = np.where(okJ, (newJ.astype(f64) - (iJ.astype(f32).astype(f64) + 0.5)).astype(f32), f32(0.5)).astype(f32)
        sI, sJ = np.where(di > 0, 1, -1), np.where(dj > 0, 1, -1)
        adi, adj = np.abs(di), np.abs(dj)
        a64, b64 = adi.astype(f64), adj.astype(f64)
        # horizontal, vertical, diagonal, self — in the reference's order
        nI, nJ = (iI + sI, iI, iI + sI, iI), (iJ, iJ + sJ, iJ + sJ, iJ)
        want = (di != 0, dj != 0, (di != 0) & (dj != 0), np.ones(len(idx), bool))
        wgt = ((a64 * (1.0 - b64)).astype(f32), (b64 * (1.0 - a64)).astype(f32), adi * adj, ((1.0 - a64) * (1.0 - b64)).astype(f32))
        inside = [wk & okI & okJ & (ni >= 0) & (ni < mw) & (nj >= 0) & (nj < mh) for wk, ni, nj in zip(want, nI, nJ)]
        at = [np.where(ins, ni + nj * mw, 0) for ins, ni, nj in zip(inside, nI, nJ)]
        wgt = [np.where(ins, wk, f32(0)).astype(f32) for ins, wk in zip(inside, wgt)]
        sumW = f32(0) + wgt[0] + wgt[1] + wgt[2] + wgt[3]
        has = sumW > 0
        out["stale"][idx] = ~has
        t = {k: st[k, idx].copy() for k in range(6, 12)}            # this cell's _Temp entries: what the previous step left
        for m in (0, 1):
            tm = [np.where(ins, wk * src[MEAN + m, a], f32(0)).astype(f32) for ins, wk, a in zip(inside, wgt, at)]
            ta = [np.where(ins, wk * src[AGE + m, a], f32(0)).astype(f32) for ins, wk, a in zip(inside, wgt, at)]
            t[MEAN_T + m] = np.where(has, (tm[0] + tm[1] + tm[2] + tm[3]) / sumW, t[MEAN_T + m]).astype(f32)
            t[AGE_T + m] = np.where(has, (ta[0] + ta[1] + ta[2] + ta[3]) / sumW, t[AGE_T + m]).astype(f32)
        for m in (0, 1):
            tv = []
            for ins, wk, a in zip(inside, wgt, at):
                d = t[MEAN_T + m] - src[MEAN + m, a]
                tv.append(np.where(ins, (wk.astype(f64) * (src[VAR + m, a].astype(f64) + 1.0 * self.square(d))).astype(f32), f32(0)).astype(f32))
            t[VAR_T + m] = np.where(has, (tv[0] + tv[1] + tv[2] + tv[3]) / sumW, t[VAR_T + m]).astype(f32)
        border = self.on_border(iI, iJ)
        for m in (0, 1):
            v = _max(t[VAR_T + m].astype(f64), MIN_BG_VAR).astype(f32)                                       # :355
            over = v.astype(f64) - VAR_MIN_NOISE_T
            arg = np.where(border, 0.0, -VAR_DEC_RATIO * _max(0.0, over))
            aged = _min(t[AGE_T + m].astype(f64) * _exp(arg), MAX_BG_AGE).astype(f32)                          # :365
            t[VAR_T + m] = np.where(border, f32(INIT_BG_VAR), v).astype(f32)                                 # :359
            t[AGE_T + m] = np.where(border, f32(0), aged).astype(f32)
            out["exp_arg"][m, idx] = arg
        # ---- update, pass 1 (:392-456) ----
        cur_mean = (px.astype(f32).sum(axis=1, dtype=f32) / f32(16.0)).astype(f32)         # (sums of 16 bytes are exact in float32)
        old_age = np.where(t[AGE_T] >= 0, t[AGE_T], f32(0))
        self.oldest_to_front(self.mode1_is_oldest(t[AGE_T + 1], old_age), t, cur_mean)
        m0 = self.square(cur_mean - t[MEAN_T]) < 2.0 * t[VAR_T].astype(f64)
        m1 = self.square(cur_mean - t[MEAN_T + 1]) < 2.0 * t[VAR_T + 1].astype(f64)
        match = np.where(m0, 0, 1)
        t[AGE_T + 1] = np.where(~m0 & ~m1, f32(0), t[AGE_T + 1]).astype(f32)
        # ---- pass 2 (:463-511) ----
        new = {}
        alpha = {}
        for m in (0, 1):
            age = t[AGE_T + m]
            alpha[m] = (age.astype(f64) / (age.astype(f64) + 1.0)).astype(f32)
            blend = ((alpha[m] * t[MEAN_T + m]).astype(f64) + (1.0 - alpha[m].astype(f64)) * cur_mean.astype(f64)).astype(f32)
            new[MEAN + m] = np.where(match == m, np.where(age < 1, cur_mean, blend), t[MEAN_T + m]).astype(f32)
        # ---- pass 3 (:512-580) ----
        p = px.astype(f32)
        mean_match = np.where(match == 0, new[MEAN], new[MEAN + 1])
        pixel_dist = (f32(0) + self.square(p - mean_match[:, None])).astype(f32)
        dist = self.square(p - new[MEAN][:, None]).astype(f32)
        obs_var = pixel_dist.max(axis=1)
        for m in (0, 1):
            age = t[AGE_T + m]
            first = _max(obs_var.astype(f64), INIT_BG_VAR).astype(f32)
            v = ((alpha[m] * t[VAR_T + m]).astype(f64) + (1.0 - alpha[m].astype(f64)) * obs_var.astype(f64)).astype(f32)
            v = _max(v.astype(f64), MIN_BG_VAR).astype(f32)
            new[VAR + m] = np.where(match == m, np.where(age == 0, first, v), t[VAR_T + m]).astype(f32)
            new[AGE + m] = np.where(match == m, _min((age.astype(f64) + 1.0).astype(f32).astype(f64), MAX_BG_AGE).astype(f32), age).astype(f32)
        var_for_mask = self.mask_variance(t[VAR_T], new[VAR])
        fg = (t[AGE_T] > 1)[:, None] & (dist.astype(f64) > 2.0 * var_for_mask.astype(f64)[:, None])
        rows = (BLOCK * j)[:, None, None] + np.arange(BLOCK)[None, :, None]
        cols = (BLOCK * i)[:, None, None] + np.arange(BLOCK)[None, None, :]
        out["dist"][rows, cols] = dist.reshape(-1, BLOCK, BLOCK)
        if out["mask"] is not None:
            out["mask"][rows, cols] = np.where(fg, 255, 0).astype(np.uint8).reshape(-1, BLOCK, BLOCK)
        for k in range(6):
            st[k, idx] = new[k]
        for k in range(6, 12):
            st[k, idx] = t[k]


def cv_round(v) -> np.ndarray:
    """cvRound of a float: to the nearest integer, halves to the even one (what cv::Mat::at(Point2f -> Point) does)."""
    return np.rint(np.asarray(v, f32).astype(f64)).astype(np.int64)


class MotionRestatement:
    """MCDWrapper::Run up to BGModel.update(detect_img), one object per tracker."""

    def __init__(self, width: int, height: int, model_class=ProbModel):
        self.model = model_class(width, height)
        self.last = None

    def step(self, image, H) -> dict:
        """image: h x w uint8 (any strides). Returns model_step's dict plus gray (the median image)."""
        gray = median5(np.asarray(image, np.uint8))
        out = self.model.model_step(gray, H)
        out["gray"] = gray
        self.last = out
        return out

    @staticmethod
    def features_on_mask(mask, feature_px, round_fn=cv_round) -> np.ndarray:
        """src/Frame.cpp:352: mask.at<uchar>(Point(cvRound(x), cvRound(y))) == 255, one flag per feature. Raises IndexError for a
        feature that rounds outside the image (the reference reads out of bounds there)."""
        f = np.asarray(feature_px, f32).reshape(-1, 2)
        x, y = round_fn(f[:, 0]), round_fn(f[:, 1])
        h, w = mask.shape
        bad = np.flatnonzero((x < 0) | (x >= w) | (y < 0) | (y >= h))
        if len(bad):
            raise IndexError(f"feature {int(bad[0])} rounds to ({int(x[bad[0]])}, {int(y[bad[0]])}), outside {w}x{h}")
        return (mask[y, x] == 255).astype(np.uint8)
