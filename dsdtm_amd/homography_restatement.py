"""RANSAC homography as THIS PROJECT defines it (include/dsdtm_amd_homography.h), restated in float64 numpy: the yardstick of
dsdtm_find_homographies (csrc/homography.hip). Its plain-C twin is tests/homography_restatement.c; the two are bit-equal
(tests/test_homography_cpu.py) and the device is bit-equal to both (tests/test_homography_gpu.py).

What is kept of cv::findHomography(A, B, CV_RANSAC) at its default arguments is its documented shape: 4-point samples, forward
reprojection error against 3 px, confidence 0.995, about 2000 hypotheses at most, a refit on the inliers of the best model, the mask
of the RANSAC model returned. Everything else is this project's definition — which samples are drawn, how ties fall, when the loop stops
and how the refit iterates. OpenCV is not available to this project in source or binary, so parity with it is unpinned.

One order of operations: every decision rests on + - * / sqrt in IEEE double, elementwise (numpy fuses nothing), sums in the fixed
shape of the kernel (256 strided partials in index order over the inliers, then a tree 128, 64, ... 1). No log, pow or exp anywhere.
The methods of Ransac that a mutant overrides (tests/test_homography_cpu.py) are the definitions a caller could trip over.
"""
from __future__ import annotations

import numpy as np

MAX_POINTS = 2048
ROUND = 256                      # hypotheses per round (= threads of the workgroup)
TREE = 256
MAX_DRAWS = 16
REFIT_ITERATIONS = 10
DEFAULT_THRESHOLD, DEFAULT_CONFIDENCE, DEFAULT_MAX_HYPOTHESES, DEFAULT_SEED = 3.0, 0.995, 2048, 0x2545F491
MAX_HYPOTHESES_CAP = 4096
SQRT2 = 1.4142135623730951
_M32 = np.uint64(0xFFFFFFFF)
f64 = np.float64


def hash3(seed, k, c):
    """The counter-based hash of (seed, hypothesis index, draw counter): uint32 arithmetic (carried in uint64, masked)."""
    k = np.asarray(k, np.uint64)
    x = (np.uint64(seed) + k * np.uint64(0x9E3779B9) + np.uint64(c) * np.uint64(0x85EBCA6B)) & _M32
    x ^= x >> np.uint64(16)
    x = (x * np.uint64(0x7FEB352D)) & _M32
    x ^= x >> np.uint64(15)
    x = (x * np.uint64(0x846CA68B)) & _M32
    x ^= x >> np.uint64(16)
    return x


def finite(v):
    with np.errstate(invalid="ignore"):
        return (v - v) == 0.0


def tree_sum(values, flags):
    """Sum of values[i] over flags[i] in the kernel's shape. values: (m,) or (q, m)."""
    v = np.atleast_2d(np.asarray(values, f64))
    m = v.shape[1]
    part = np.zeros((v.shape[0], TREE), f64)
    for j in range(0, m, TREE):
        n = min(TREE, m - j)
        with np.errstate(invalid="ignore", over="ignore"):
            part[:, :n] = np.where(flags[j:j + n][None, :], part[:, :n] + v[:, j:j + n], part[:, :n])
    stride = TREE // 2
    with np.errstate(invalid="ignore", over="ignore"):
        while stride >= 1:
            part[:, :stride] = part[:, :stride] + part[:, stride:2 * stride]
            stride //= 2
    out = part[:, 0].copy()
    return out if np.ndim(values) == 2 else out[0]


def mul3(a, b):
    c = [0.0] * 9
    for i in range(3):
        for j in range(3):
            c[3 * i + j] = (a[3 * i] * b[j] + a[3 * i + 1] * b[3 + j]) + a[3 * i + 2] * b[6 + j]
    return c


def adj3(m):
    return [m[4] * m[8] - m[5] * m[7], m[2] * m[7] - m[1] * m[8], m[1] * m[5] - m[2] * m[4],
            m[5] * m[6] - m[3] * m[8], m[0] * m[8] - m[2] * m[6], m[2] * m[3] - m[0] * m[5],
            m[3] * m[7] - m[4] * m[6], m[1] * m[6] - m[0] * m[7], m[0] * m[4] - m[1] * m[3]]


def normalise(H):
    """H / H[8] and whether that is usable (H[8] neither zero nor non-finite, every entry finite). Entries: scalars or arrays."""
    with np.errstate(all="ignore"):
        s = H[8]
        out = [h / s for h in H]
        ok = (s != 0.0) & finite(s)
        for h in out:
            ok = ok & finite(h)
    return out, ok


def basis(x, y):
    """The projective basis of four points (x[i], y[i] arrays over the hypotheses): columns lambda_i (x_i, y_i, 1)."""
    with np.errstate(all="ignore"):
        a00, a01, a02 = y[1] - y[2], x[2] - x[1], x[1] * y[2] - x[2] * y[1]
        a10, a11, a12 = y[2] - y[0], x[0] - x[2], x[2] * y[0] - x[0] * y[2]
        a20, a21, a22 = y[0] - y[1], x[1] - x[0], x[0] * y[1] - x[1] * y[0]
        det = (a02 + a12) + a22
        l0 = ((a00 * x[3] + a01 * y[3]) + a02) / det
        l1 = ((a10 * x[3] + a11 * y[3]) + a12) / det
        l2 = ((a20 * x[3] + a21 * y[3]) + a22) / det
        M = [l0 * x[0], l1 * x[1], l2 * x[2], l0 * y[0], l1 * y[1], l2 * y[2], l0, l1, l2]
        ok = (det != 0.0) & finite(det)
        for l in (l0, l1, l2):
            ok = ok & (l != 0.0) & finite(l)
    return M, ok


def gn_terms(h, c, ax, ay, bx, by):
    """The 30 terms per point of one Gauss-Newton evaluation at h (h[8] = 1), c = (cxa, cya, cxb, cyb, sa, sb)."""
    with np.errstate(all="ignore"):
        x, y, bu, bv = (ax - c[0]) * c[4], (ay - c[1]) * c[4], (bx - c[2]) * c[5], (by - c[3]) * c[5]
        w = (h[6] * x + h[7] * y) + 1.0
        u, v = ((h[0] * x + h[1] * y) + h[2]) / w, ((h[3] * x + h[4] * y) + h[5]) / w
        ru, rv = u - bu, v - bv
        iw = 1.0 / w
        a, b, cc = x * iw, y * iw, iw
        p6, p7, q6, q7 = u * a, u * b, v * a, v * b
        return np.stack([a * a, a * b, a * cc, b * b, b * cc, cc * cc,
                         a * p6, a * p7, b * p6, b * p7, cc * p6, cc * p7,
                         a * q6, a * q7, b * q6, b * q7, cc * q6, cc * q7,
                         p6 * p6 + q6 * q6, p6 * p7 + q6 * q7, p7 * p7 + q7 * q7,
                         a * ru, b * ru, cc * ru, a * rv, b * rv, cc * rv,
                         p6 * ru + q6 * rv, p7 * ru + q7 * rv, ru * ru + rv * rv])


def solve_step(S):
    """J^T J x = J^T r by Cholesky from the 30 sums. None at a non-positive pivot or a non-finite entry."""
    S = [float(s) for s in S]
    A = [[0.0] * 8 for _ in range(8)]
    A[0][0], A[0][1], A[0][2], A[1][1], A[1][2], A[2][2] = S[0:6]
    A[3][3], A[3][4], A[3][5], A[4][4], A[4][5], A[5][5] = S[0:6]
    A[0][6], A[0][7], A[1][6], A[1][7], A[2][6], A[2][7] = [-s for s in S[6:12]]
    A[3][6], A[3][7], A[4][6], A[4][7], A[5][6], A[5][7] = [-s for s in S[12:18]]
    A[6][6], A[6][7], A[7][7] = S[18:21]
    g = S[21:27] + [-S[27], -S[28]]
    L = [[0.0] * 8 for _ in range(8)]
    with np.errstate(all="ignore"):
        for j in range(8):
            s = f64(A[j][j])
            for k in range(j):
                s = s - L[j][k] * L[j][k]
            if not (s > 0.0) or not finite(s):
                return None
            L[j][j] = np.sqrt(s)
            for i in range(j + 1, 8):
                t = f64(A[j][i])
                for k in range(j):
                    t = t - L[i][k] * L[j][k]
                L[i][j] = t / L[j][j]
        yv, x = [f64(0.0)] * 8, [f64(0.0)] * 8
        for i in range(8):
            s = f64(g[i])
            for k in range(i):
                s = s - L[i][k] * yv[k]
            yv[i] = s / L[i][i]
        ok = True
        for i in range(7, -1, -1):
            s = yv[i]
            for k in range(i + 1, 8):
                s = s - L[k][i] * x[k]
            x[i] = s / L[i][i]
            ok = ok and bool(finite(x[i]))
    return x if ok else None


class Ransac:
    """The definition. find(A, B, ...) returns dict(found, H, H_ransac, mask, n_inliers, best_hypothesis, rounds, refit_iterations,
    cost_before, cost_after); found == 0 carries nothing else."""

    # ---- the definitions a caller could trip over (each is a mutant in the tests) ----
    def runs(self, m):
        return m > 4                                   # the reference's tPointsA.size() > 4

    def within(self, d2, thr2):
        return d2 <= thr2

    def pick(self, counts):
        return int(np.argmax(counts))                  # ties go to the LOWEST hypothesis index

    def oriented(self, A, B):
        return A, B                                    # H maps A (current frame) to B (last frame)

    def redraw(self):
        return True

    def refits(self):
        return True

    def returned_mask(self, ransac_mask, refit_mask):
        return ransac_mask                             # the RANSAC model's, not re-evaluated after the refit

    def stop_inside_round(self, counts, k0, best_count, m, left):
        return None                                    # the stop rule is evaluated per ROUND

    # ---- the parts ----
    def samples(self, seed, k, m):
        """(4, n) indices and validity for the hypotheses k."""
        n = len(k)
        s = np.zeros((4, n), np.int64)
        got = np.zeros(n, np.int64)
        for c in range(MAX_DRAWS):
            i = ((hash3(seed, k, c) * np.uint64(m)) >> np.uint64(32)).astype(np.int64)
            fresh = got < 4
            if self.redraw():
                for j in range(4):
                    fresh &= ~((j < got) & (s[j] == i))
            for j in range(4):
                put = fresh & (got == j)
                s[j] = np.where(put, i, s[j])
            got = got + fresh
        return s, got == 4

    def solve(self, ax, ay, bx, by, s):
        A, okA = basis([ax[s[i]] for i in range(4)], [ay[s[i]] for i in range(4)])
        B, okB = basis([bx[s[i]] for i in range(4)], [by[s[i]] for i in range(4)])
        with np.errstate(all="ignore"):
            H = mul3(B, adj3(A))
        H, okH = normalise(H)
        return H, okA & okB & okH

    def inliers(self, H, ax, ay, bx, by, thr2):
        """H: 9 scalars or 9 arrays (n,) -> flags (m,) or (n, m)."""
        h = [np.asarray(v, f64)[..., None] for v in H]
        with np.errstate(all="ignore"):
            w = (h[6] * ax + h[7] * ay) + h[8]
            px, py = ((h[0] * ax + h[1] * ay) + h[2]) / w, ((h[3] * ax + h[4] * ay) + h[5]) / w
            dx, dy = bx - px, by - py
            return self.within(dx * dx + dy * dy, thr2)

    def refit(self, ax, ay, bx, by, flags, n_in, H):
        """-> (H, iterations, cost_before, cost_after)"""
        with np.errstate(all="ignore"):
            c = list(tree_sum(np.stack([ax, ay, bx, by]), flags) / f64(n_in))
            da = np.sqrt((ax - c[0]) * (ax - c[0]) + (ay - c[1]) * (ay - c[1]))
            db = np.sqrt((bx - c[2]) * (bx - c[2]) + (by - c[3]) * (by - c[3]))
            s2 = tree_sum(np.stack([da, db]), flags)
            c += [f64(SQRT2) / (s2[0] / f64(n_in)), f64(SQRT2) / (s2[1] / f64(n_in))]
            scales_ok = c[4] > 0.0 and finite(c[4]) and c[5] > 0.0 and finite(c[5])
            one, zero = f64(1.0), f64(0.0)
            Tb = [c[5], zero, -(c[5] * c[2]), zero, c[5], -(c[5] * c[3]), zero, zero, one]
            Tai = [one / c[4], zero, c[0], zero, one / c[4], c[1], zero, zero, one]
            h, ok = normalise(mul3(Tb, mul3([f64(v) for v in H], Tai)))
            if not scales_ok or not ok:
                return H, 0, 0.0, 0.0
            S = tree_sum(gn_terms(h, c, ax, ay, bx, by), flags)
            sb2 = c[5] * c[5]
            before = S[29] / sb2
            it = 0
            for _ in range(REFIT_ITERATIONS):
                x = solve_step(S)
                if x is None:
                    break
                t = [h[i] - x[i] for i in range(8)] + [one]
                S2 = tree_sum(gn_terms(t, c, ax, ay, bx, by), flags)
                if not (S2[29] < S[29]):
                    break
                h, S, it = t, S2, it + 1
            if it == 0:
                return H, 0, float(before), float(before)
            Tbi = [one / c[5], zero, c[2], zero, one / c[5], c[3], zero, zero, one]
            Ta = [c[4], zero, -(c[4] * c[0]), zero, c[4], -(c[4] * c[1]), zero, zero, one]
            Hn, ok = normalise(mul3(Tbi, mul3(h, Ta)))
            if not ok:
                return H, 0, float(before), float(before)
            return [float(v) for v in Hn], it, float(before), float(S[29] / sb2)

    def find(self, A, B, thr=DEFAULT_THRESHOLD, confidence=DEFAULT_CONFIDENCE, max_hypotheses=DEFAULT_MAX_HYPOTHESES, seed=DEFAULT_SEED):
        A, B = self.oriented(np.asarray(A, np.float32).reshape(-1, 2), np.asarray(B, np.float32).reshape(-1, 2))
        m = len(A)
        if not self.runs(m) or m > MAX_POINTS:
            return dict(found=0)
        ax, ay, bx, by = A[:, 0].astype(f64), A[:, 1].astype(f64), B[:, 0].astype(f64), B[:, 1].astype(f64)
        thr2, left = f64(thr) * f64(thr), f64(1.0) - f64(confidence)
        rounds_max = (int(max_hypotheses) + ROUND - 1) // ROUND
        best_count, best_k, best_H, rounds = -1, -1, None, 0
        for r in range(rounds_max):
            k = np.arange(r * ROUND, (r + 1) * ROUND, dtype=np.uint64)
            s, drawn = self.samples(seed, k, m)
            H, solved = self.solve(ax, ay, bx, by, s)
            counts = np.where(drawn & solved, self.inliers(H, ax, ay, bx, by, thr2).sum(axis=1), -1)
            cut = self.stop_inside_round(counts, r * ROUND, best_count, m, left)
            if cut is not None:
                counts = np.where(np.arange(ROUND) <= cut, counts, -2)
            l = self.pick(counts)
            if counts[l] > best_count:
                best_count, best_k, best_H = int(counts[l]), r * ROUND + l, [float(h[l]) for h in H]
            rounds = r + 1
            cnt = max(best_count, 0)
            if cnt == m or cut is not None:
                break
            w = f64(cnt) / f64(m)
            q = f64(1.0) - (w * w) * (w * w)
            p = q
            for _ in range(8):
                p = p * p
            t = p
            for _ in range(1, rounds):
                t = t * p
            if t <= left:
                break
        if best_count < 4:
            return dict(found=0)
        flags = self.inliers(best_H, ax, ay, bx, by, thr2)
        Hr, it, before, after = (self.refit(ax, ay, bx, by, flags, best_count, best_H) if self.refits() else (best_H, 0, 0.0, 0.0))
        mask = self.returned_mask(flags, self.inliers(Hr, ax, ay, bx, by, thr2))
        return dict(found=1, H=np.array(Hr, f64), H_ransac=np.array(best_H, f64), mask=mask.astype(np.uint8), n_inliers=best_count,
                    best_hypothesis=best_k, rounds=rounds, refit_iterations=it, cost_before=before, cost_after=after)


def find_homography(A, B, thr=DEFAULT_THRESHOLD, confidence=DEFAULT_CONFIDENCE, max_hypotheses=DEFAULT_MAX_HYPOTHESES, seed=DEFAULT_SEED):
    return Ransac().find(A, B, thr, confidence, max_hypotheses, seed)
