"""The contour step of MCDWrapper::Run (Thirdparty/fastMCD/src/MCDWrapper.cpp:98-128) restated: rules C1-C6 of include/dsdtm_amd_mcd.h.

A plain sequential restatement — a raster scan, a flood fill and a Moore trace per component, no pruning, no union-find — and the
yardstick for tests/contour_restatement.c (its plain-C twin), mcd_box_host (dsdtm_amd/host/dsdtm_mcd_host.hpp) and the device
(csrc/contour.hip), all bit-equal to it. Integer only. Parity with OpenCV's findContours is unpinned (see the header).

    r = ContourRestatement().run(mask)      # dict(box, area2, n_components, boxed, components)
"""
from __future__ import annotations

import numpy as np

# directions as OpenCV's border follower numbers them: 0 = E, then counter-clockwise on the screen (y grows downwards)
DX = (1, 1, 0, -1, -1, -1, 0, 1)
DY = (0, -1, -1, -1, 0, 1, 1, 1)


class ContourRestatement:
    """C1-C5. A subclass that overrides CONNECTIVITY, beats or rect is a mutant (tests/test_mcd_cpu.py tells them apart)."""
    CONNECTIVITY = 8

    def foreground(self, mask):
        """C1: non-zero bytes."""
        return np.asarray(mask) != 0

    def beats(self, area2, best):
        """C4: `area > maxArea` (:112), from 0."""
        return area2 > best

    def rect(self, minx, miny, maxx, maxy):
        """C5: the rows and columns filled, both ends inclusive."""
        return slice(miny, maxy + 1), slice(minx, maxx + 1)

    def components(self, fg):
        """The components in raster order of their first pixel: (roots, labels). A pixel's label is its component's root (the index
        y * w + x of its raster-first pixel); background is -1."""
        h, w = fg.shape
        label = np.full((h, w), -1, np.int64)
        steps = [(dx, dy) for dx, dy in zip(DX, DY) if self.CONNECTIVITY == 8 or dx == 0 or dy == 0]
        roots = []
        for p in np.flatnonzero(fg):
            y, x = divmod(int(p), w)
            if label[y, x] >= 0:
                continue
            roots.append(int(p))
            label[y, x] = p
            stack = [(x, y)]
            while stack:
                cx, cy = stack.pop()
                for dx, dy in steps:
                    nx, ny = cx + dx, cy + dy
                    if 0 <= nx < w and 0 <= ny < h and fg[ny, nx] and label[ny, nx] < 0:
                        label[ny, nx] = p
                        stack.append((nx, ny))
        return roots, label

    @staticmethod
    def trace(fg, x0, y0):
        """C2: the outer border of the component whose raster-first pixel is (x0, y0), as a list of (x, y)."""
        h, w = fg.shape

        def on(x, y):
            return 0 <= x < w and 0 <= y < h and bool(fg[y, x])

        s = 4                                   # entered from the left neighbour
        while True:                             # clockwise from there: the walk's last pixel
            s = (s - 1) & 7
            if on(x0 + DX[s], y0 + DY[s]) or s == 4:
                break
        if s == 4:
            return [(x0, y0)]
        x1, y1 = x0 + DX[s], y0 + DY[s]
        points, x, y = [], x0, y0
        for _ in range(4 * h * w + 4):
            while True:                         # counter-clockwise behind the pixel it was entered from
                s = (s + 1) & 7
                nx, ny = x + DX[s], y + DY[s]
                if on(nx, ny):
                    break
            points.append((x, y))
            if (nx, ny) == (x0, y0) and (x, y) == (x1, y1):        # Suzuki's stop: about to repeat the first move
                return points
            x, y, s = nx, ny, (s + 4) & 7
        raise RuntimeError("a contour walk passed its cap of 4 * pixels + 4 steps")

    @staticmethod
    def area2(points):
        """C3: |sum x_prev * y_cur - y_prev * x_cur| over the closed walk (Python integers)."""
        acc, (px, py) = 0, points[-1]
        for x, y in points:
            acc += px * y - py * x
            px, py = x, y
        return abs(acc)

    def run(self, mask):
        mask = np.ascontiguousarray(mask, np.uint8)
        fg = self.foreground(mask)
        roots, label = self.components(fg)
        comps, best, winner = [], 0, None
        w = mask.shape[1]
        for root in roots:
            pts = self.trace(fg, root % w, root // w)
            xs, ys = [p[0] for p in pts], [p[1] for p in pts]
            c = dict(root=root, area2=self.area2(pts), minx=min(xs), miny=min(ys), maxx=max(xs), maxy=max(ys), points=len(pts))
            comps.append(c)
            if self.beats(c["area2"], best):
                best, winner = c["area2"], c
        boxed = mask.copy()
        box = [0, 0, 0, 0]
        if winner is not None:
            boxed[self.rect(winner["minx"], winner["miny"], winner["maxx"], winner["maxy"])] = 255
            box = [winner["minx"], winner["miny"], winner["maxx"] - winner["minx"] + 1, winner["maxy"] - winner["miny"] + 1]
        return dict(box=box, area2=int(winner["area2"]) if winner is not None else 0, n_components=len(roots), boxed=boxed, components=comps,
                    labels=label)


def box_mask(mask):
    """C1-C5 on one mask: (box [x, y, w, h], area2, n_components, the mask with the rectangle)."""
    r = ContourRestatement().run(mask)
    return r["box"], r["area2"], r["n_components"], r["boxed"]


def features_on_mask(boxed, px):
    """C6: the test of Frame::Motion_Removal (src/Frame.cpp:352) on the image with the rectangle: cvRound (halves to even), == 255."""
    px = np.asarray(px, np.float32).reshape(-1, 2)
    x, y = np.rint(px[:, 0]).astype(np.int64), np.rint(px[:, 1]).astype(np.int64)
    return (boxed[y, x] == 255).astype(np.uint8)
