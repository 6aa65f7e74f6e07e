"""The numpy yardstick of libdsdtm_amd_clahe.so: rules E1-E6 of include/dsdtm_amd_clahe.h (cv::CLAHE::apply for CV_8UC1 in the shape of
OpenCV 2.4; everything finer is this project's definition, and parity with OpenCV binaries is unpinned). Float32 arithmetic is
explicit (np.float32 operands, one operation per expression), and the extended image of E1 is MATERIALISED with np.pad, so that the
yardstick is independent of the index reflection the device and the host function use.

The class has one method per rule, so that a test can replace one rule by a mutant and see a case tell it apart."""
from __future__ import annotations

import numpy as np

MIN_SIDE, MAX_SIDE, MAX_TILES, DEFAULT_TILES, DEFAULT_CLIP_LIMIT, MAX_FRAMES = 16, 4096, 16, 8, 3.0, 1024
F = np.float32


class Clahe:
    def __init__(self, clip_limit=DEFAULT_CLIP_LIMIT, tiles_x=DEFAULT_TILES, tiles_y=DEFAULT_TILES):
        self.clip_limit, self.tiles_x, self.tiles_y = float(clip_limit), int(tiles_x) or DEFAULT_TILES, int(tiles_y) or DEFAULT_TILES

    # E1
    def padding(self, width, height):
        """(columns added on the right, rows added at the bottom)"""
        if width % self.tiles_x == 0 and height % self.tiles_y == 0:
            return 0, 0
        return self.tiles_x - width % self.tiles_x, self.tiles_y - height % self.tiles_y

    def extended(self, img):
        px, py = self.padding(img.shape[1], img.shape[0])
        return np.pad(img, ((0, py), (0, px)), mode="reflect") if (px or py) else img

    # E2
    def clip(self, area):
        """0: no clipping"""
        if not self.clip_limit > 0:
            return 0
        q = self.clip_limit * float(area) / 256.0
        return max(area if q >= area else int(q), 1)

    # E4
    def redistribute(self, h, clip):
        excess = np.maximum(h - clip, 0)
        clipped = int(excess.sum())
        h = np.minimum(h, clip)
        batch = clipped // 256
        residual = clipped - 256 * batch
        h = h + batch
        h[:residual] += 1
        return h

    # E5
    def round_u8(self, v):
        """saturate_u8(cvRound(v)) of float32 values: halves to even"""
        return np.clip(np.rint(v), 0, 255).astype(np.uint8)

    def table(self, h, area):
        scale = F(255.0) / F(area)
        return self.round_u8(np.cumsum(h, dtype=np.int32).astype(F) * scale)

    def luts(self, img):
        """(tiles_y, tiles_x, 256) uint8"""
        ext = self.extended(img)
        tw, th = ext.shape[1] // self.tiles_x, ext.shape[0] // self.tiles_y
        area = tw * th
        clip = self.clip(area)
        out = np.empty((self.tiles_y, self.tiles_x, 256), np.uint8)
        for ty in range(self.tiles_y):
            for tx in range(self.tiles_x):
                tile = ext[ty * th:(ty + 1) * th, tx * tw:(tx + 1) * tw]
                h = np.bincount(tile.ravel(), minlength=256).astype(np.int32)          # E3
                if clip > 0:
                    h = self.redistribute(h, clip)
                out[ty, tx] = self.table(h, area)
        return out

    # E6
    def axis(self, n, tile, tiles):
        """(t1, t2, a) for the positions 0 .. n-1 of one axis"""
        inv = F(1.0) / F(tile)
        f = np.arange(n, dtype=F) * inv - F(0.5)
        fl = np.floor(f)
        a = f - fl
        i = fl.astype(np.int32)
        return np.maximum(i, 0), np.minimum(i + 1, tiles - 1), a

    def blend(self, p11, p12, p21, p22, xa, ya):
        one = F(1.0)
        res = p11 * ((one - xa) * (one - ya))
        res = res + p12 * (xa * (one - ya))
        res = res + p21 * ((one - xa) * ya)
        res = res + p22 * (xa * ya)
        return res

    def interpolate(self, img, luts):
        h, w = img.shape
        px, py = self.padding(w, h)
        x1, x2, xa = self.axis(w, (w + px) // self.tiles_x, self.tiles_x)
        y1, y2, ya = self.axis(h, (h + py) // self.tiles_y, self.tiles_y)
        v = img.astype(np.intp)
        Y1, Y2, YA = y1[:, None], y2[:, None], ya[:, None]
        X1, X2, XA = x1[None, :], x2[None, :], xa[None, :]
        res = self.blend(luts[Y1, X1, v].astype(F), luts[Y1, X2, v].astype(F), luts[Y2, X1, v].astype(F), luts[Y2, X2, v].astype(F), XA, YA)
        assert res.dtype == F
        return self.round_u8(res)

    def apply(self, img):
        """(equalised image, luts)"""
        img = np.asarray(img)
        assert img.dtype == np.uint8 and img.ndim == 2
        luts = self.luts(img)
        return self.interpolate(img, luts), luts


def clahe(img, clip_limit=DEFAULT_CLIP_LIMIT, tiles_x=DEFAULT_TILES, tiles_y=DEFAULT_TILES, cls=Clahe):
    """The equalised image of E1-E6."""
    return cls(clip_limit, tiles_x, tiles_y).apply(img)[0]


def clahe_luts(img, clip_limit=DEFAULT_CLIP_LIMIT, tiles_x=DEFAULT_TILES, tiles_y=DEFAULT_TILES, cls=Clahe):
    return cls(clip_limit, tiles_x, tiles_y).luts(np.asarray(img))
