"""Case builders for the detector's batch entry (dsdtm_detect_cells_batch_device), shared by tests/test_detector_cases_cpu.py
(holds every case to its conditions with the oracle alone) and tests/test_detector_paths_gpu.py (runs them on the device).

A case is a level table (width, height, stride, level_offset, pyr_pitch: the caller's, not necessarily the packed layout of
capi.pyramid_layout), n frames of level images (the batch entry takes the pyramid's bytes as given, so the levels of a frame need
not be pyrDown of each other: most cases give every level a texture of its own, so that every level decides cells), a per-frame
occupancy grid and the detector parameters. Each case names the kernels its geometry is meant to reach; kernel_paths() restates
the launcher's rule (detect.hip, detect_launch) ONLY to guard this table against a later edit of a shape — it is no oracle.

Nothing here imports the GPU."""
from __future__ import annotations

import dataclasses
import functools

import numpy as np

from dsdtm_amd import capi, synth
from tests import helpers as H

CELL = 25                 # Camera.CellSize of the reference's configuration; the small cases use it too
BARRIER, THRESHOLD = 20, 5.0


@dataclasses.dataclass
class Case:
    name: str
    width: tuple
    height: tuple
    stride: tuple
    offset: tuple
    pitch: int
    images: list              # images[frame][level]: (height[l], width[l]) uint8
    occ: np.ndarray           # (n, grid_cols * grid_rows) uint8
    grid_cols: int
    grid_rows: int
    score: tuple              # per level: "strip" | "pixel" — the score kernel the level is meant to take
    select: str               # "rows" | "select4" | "select1" — the select kernel of the whole batch
    sub_n: int | None = None  # the first sub_n frames run as a batch of their own as well ...
    sub_select: str = "select1"   # ... and are meant to take this select kernel
    cell_size: int = CELL
    barrier: int = BARRIER
    threshold: float = THRESHOLD
    twin: str | None = None   # a case with the same images, occupancy and parameters in another layout: the cells must be equal

    @property
    def n(self):
        return len(self.images)

    @property
    def levels(self):
        return len(self.width)

    @property
    def cells(self):
        return self.grid_cols * self.grid_rows


# ---- the launcher's rule, restated ------------------------------------------------------------------------------------------
def kernel_paths(width, stride, offset, pitch, n):
    """(per-level score kernel, select kernel) a geometry reaches: a level takes the strip kernel iff width, stride and offset are
    multiples of 4, the width is >= 16 and the pitch is a multiple of 4; the select pass is the rows kernel iff n >= 8 and no
    level takes the per-pixel kernel, otherwise select<4> for n >= 8 and select<1> below."""
    score = tuple("strip" if ((w | s | o) & 3) == 0 and w >= 16 and (pitch & 3) == 0 else "pixel" for w, s, o in zip(width, stride, offset))
    if n >= 8:
        return score, ("rows" if "pixel" not in score else "select4")
    return score, "select1"


def strip_workgroups(w, h):
    """workgroups of 256 tasks a strip level needs (score and rows kernel alike: one task per 4 columns x 4 rows)"""
    return ((w // 4) * ((h + 3) // 4) + 255) // 256


# ---- layouts ---------------------------------------------------------------------------------------------------------------
def halves(w, h, levels):
    out = []
    for _ in range(levels):
        out.append((w, h))
        w, h = (w + 1) // 2, (h + 1) // 2
    return out


def packed_table(sizes, align=64, pitch_align=256):
    """the packed layout of capi.pyramid_layout for any list of level sizes: stride == width, offsets multiples of `align`"""
    off, offs = 0, []
    for w, h in sizes:
        offs.append(off)
        off += (w * h + align - 1) // align * align
    return tuple(w for w, _ in sizes), tuple(h for _, h in sizes), tuple(w for w, _ in sizes), tuple(offs), (off + pitch_align - 1) // pitch_align * pitch_align


def strided_table(sizes, strides, first=0, gap=0, mod=4, pitch_align=4, offsets=None):
    """levels one after the other with the given strides; every offset is rounded up to `mod` after a gap of `gap` bytes"""
    off, offs = first, []
    for i, ((w, h), s) in enumerate(zip(sizes, strides)):
        if offsets is not None and offsets[i] is not None:
            off = offsets[i]
        offs.append(off)
        off = (off + s * h + gap + mod - 1) // mod * mod
    end = max(o + s * h for o, s, (_, h) in zip(offs, strides, sizes))
    return tuple(w for w, _ in sizes), tuple(h for _, h in sizes), tuple(strides), tuple(offs), (end + pitch_align - 1) // pitch_align * pitch_align


# ---- images ----------------------------------------------------------------------------------------------------------------
def texture(h, w, seed):
    return np.clip(np.rint(synth.make_texture(h, w, seed)), 0, 255).astype(np.uint8)


def texture_levels(sizes, seed):
    """one texture per level (the levels are NOT pyrDown of each other: every level has corners that win cells)"""
    return [texture(h, w, seed + 1000 * l) for l, (w, h) in enumerate(sizes)]


def tiling(h, w, period, seed, values):
    """a (period x period) tile of 2 x 2 blocks of `values`, repeated over the image: identical corners recur every `period`
    pixels, and the pixels of a block share their value, so equal FAST scores sit side by side"""
    rng = np.random.default_rng(seed)
    tile = np.kron(rng.choice(np.array(values, np.uint8), (period // 2, period // 2)), np.ones((2, 2), np.uint8))
    return np.tile(tile, (h // period + 1, w // period + 1))[:h, :w].copy()


def checkerboard(h, w, square=4):
    yy, xx = np.mgrid[0:h, 0:w]
    return ((((yy // square) + (xx // square)) & 1) * 255).astype(np.uint8)


def random_occupancy(n, cells, share, seed):
    return (np.random.default_rng(seed).random((n, cells)) < share).astype(np.uint8)


def grid_of(w, h, cell=CELL):
    return -(-w // cell), -(-h // cell)


# ---- packing ---------------------------------------------------------------------------------------------------------------
def pack(case, n=None, seed=12345):
    """the (n, pitch) byte array of the first n frames: every byte that belongs to no level's w x h pixels — row padding, gaps
    between levels, the tail — is random"""
    n = case.n if n is None else n
    out = np.random.default_rng(seed).integers(0, 256, (n, case.pitch), dtype=np.uint8)
    for i in range(n):
        for l in range(case.levels):
            w, h, s, o = case.width[l], case.height[l], case.stride[l], case.offset[l]
            img = case.images[i][l]
            assert img.shape == (h, w) and img.dtype == np.uint8
            rows = np.lib.stride_tricks.as_strided(out[i, o:], (h, w), (s, 1))
            rows[...] = img
    return out


def table_is_valid(case):
    """what the batch entry asks of a table, plus no two levels overlapping (rows of one level may not overlap either)"""
    used = np.zeros(case.pitch, np.int32)
    for w, h, s, o in zip(case.width, case.height, case.stride, case.offset):
        if w <= 0 or h <= 0 or s < w or o + s * h > case.pitch:
            return False
        for y in range(h):
            used[o + y * s:o + y * s + w] += 1
    return case.pitch % 4 == 0 and used.max() == 1


def params(case, threshold=None):
    return capi.DetectParams(case.cell_size, case.grid_cols, case.grid_rows, case.levels, case.barrier,
                             case.threshold if threshold is None else float(threshold))


_ORACLE_CELLS = {}


def oracle_cells(oracle, case, frame, threshold=None):
    """the expected cells of one frame: oracle.detect_cells on the level images (computed once per session; read-only). Inside
    `oracle_lib.mutant(...)` the library is the mutation build whichever mutant is switched on: the switch is part of the key."""
    thr = np.float32(case.threshold if threshold is None else threshold)
    lib = oracle.load()
    key = (case.name, frame, float(thr), id(lib), lib.oracle_get_mutant() if hasattr(lib, "oracle_get_mutant") else 0)
    if key not in _ORACLE_CELLS:
        got = oracle.detect_cells(case.images[frame], case.levels, case.cell_size, case.grid_cols, case.grid_rows, case.occ[frame], thr, case.barrier)
        for a in got:
            a.setflags(write=False)
        _ORACLE_CELLS[key] = got
    return _ORACLE_CELLS[key]


def threshold_pair(oracle, case, frame=0):
    """(cell, s, the float below s): s is the winning score of a cell of `frame` with a winner — the median one, so that cells
    lie on both sides of it. With detection_threshold = s that cell's corner is no longer strictly above the threshold."""
    sc = oracle_cells(oracle, case, frame)[0]
    won = np.nonzero(sc > np.float32(case.threshold))[0]
    k = int(won[np.argsort(sc[won], kind="stable")[len(won) // 2]])
    s = np.float32(sc[k])
    return k, s, np.nextafter(s, np.float32(0))


def survivors(oracle, case, frame):
    """(level, x, y) of every corner of the frame that survives the 3x3 non-maximum step, in the reference's order"""
    out = []
    for l in range(case.levels):
        lst = oracle.fast10_list(case.images[frame][l], case.barrier)
        out += [(l, int(x), int(y)) for x, y, _, keep in lst if keep]
    return out


# ---- the cases -------------------------------------------------------------------------------------------------------------
def _case(name, table, images, grid, occ_share=0.1, **kw):
    width, height, stride, offset, pitch = table
    gc, gr = grid
    occ = kw.pop("occ", None)
    if occ is None:
        occ = random_occupancy(len(images), gc * gr, occ_share, sum(map(ord, name)))
    return Case(name=name, width=width, height=height, stride=stride, offset=offset, pitch=pitch, images=images, occ=occ,
                grid_cols=gc, grid_rows=gr, **kw)


# 1. mixed pyramids: fast_select_kernel<4> (n = 8), the first 7 frames again through fast_select_kernel<1>
def _mixed(name, w, h, levels, score):
    sizes = halves(w, h, levels)
    images = [texture_levels(sizes, 100 * i + w) for i in range(8)]
    return _case(name, packed_table(sizes), images, grid_of(w, h), score=score, select="select4", sub_n=7)


def _production():
    from dsdtm_amd.feature_detection import Feature_detector
    from dsdtm_amd.frame import Config
    old = Config.Get("Camera.MaxPyraLevels")
    Config.Set("Camera.MaxPyraLevels", 4)
    try:
        det = Feature_detector(752, 480)
    finally:
        Config.Set("Camera.MaxPyraLevels", old)
    imgs = [np.load(H.golden_path("fast_reference.npz"))["test1"]] + [texture(480, 752, 900 + i) for i in range(1, 8)]
    images = [synth.build_pyramid(im, 4) for im in imgs]         # the real pyramids of a production batch
    return _case("production_752x480", packed_table(halves(752, 480, 4)), images, (det.mGrid_cols, det.mGrid_rows),
                 score=("strip", "strip", "strip", "pixel"), select="select4", cell_size=det.mCell_size)


# 2. grid widths for det_block_x: all levels whole dwords, rows kernel at n = 9, select<1> (and the strip score kernel) at n = 3
GRID_SIZES = {(64, 60): 1, (96, 64): 2, (128, 80): 3, (176, 100): 5, (208, 128): 7, (240, 150): 9}      # level 0: workgroups of 256


def _grid_width(w, h):
    sizes = halves(w, h, 3)
    images = [texture_levels(sizes, 100 * i + w + h) for i in range(9)]
    return _case(f"grid_{w}x{h}", packed_table(sizes), images, grid_of(w, h), score=("strip",) * 3, select="rows", sub_n=3)


# 3. caller strides and offsets: 176x100, 3 levels, n = 8 and n = 2, the same images as `stride_packed`
S176 = halves(176, 100, 3)


@functools.lru_cache(maxsize=None)
def _stride_images():
    return [texture_levels(S176, 100 * i + 31) for i in range(8)]


def _strided(name, table, score, select):
    return _case(name, table, _stride_images(), grid_of(176, 100), occ=random_occupancy(8, 32, 0.1, 3), score=score, select=select,
                 sub_n=2, twin=None if name == "stride_packed" else "stride_packed")


def _tight_table():
    t = strided_table(S176, (176, 88, 44), mod=4)
    assert t[4] == t[3][2] + 44 * 25 and t[4] % 8 == 4          # ends on the last byte of the pitch; a multiple of 4 and nothing more
    return t


# 4. ties: tilings of one small tile on levels 0 and 1 (the same tiling: a cell's best score is reached on two levels), a texture
# on level 2; frame 1 is an ordinary texture. (period, seed, values) per tie frame, chosen so that the counts the CPU test asserts hold
TIE_FRAMES = [(8, 0, (10, 90, 170, 250)), None, (10, 0, (0, 255)), (12, 2, (10, 90, 170, 250)), (14, 1, (0, 255)),
              (16, 0, (10, 90, 170, 250)), (10, 3, (10, 90, 170, 250)), (12, 3, (0, 255))]


def _ties(name, w, score, select):
    sizes = halves(w, 100, 3)
    images = []
    for i, t in enumerate(TIE_FRAMES):
        if t is None:
            images.append(texture_levels(sizes, 555))
        else:
            period, seed, values = t
            images.append([tiling(sizes[0][1], sizes[0][0], period, seed, values), tiling(sizes[1][1], sizes[1][0], period, seed, values),
                           texture(sizes[2][1], sizes[2][0], 77 + i)])
    return _case(name, packed_table(sizes), images, grid_of(w, 100), occ=np.zeros((8, 32), np.uint8), score=score, select=select, sub_n=2)


# 6. frames that differ in kind inside one batch (128x80, 3 levels, n = 8)
def _kinds():
    sizes = halves(128, 80, 3)
    G = 6 * 4
    tex = texture_levels(sizes, 4242)
    flat = [np.full((h, w), 117, np.uint8) for w, h in sizes]
    chk = [checkerboard(h, w) for w, h in sizes]
    blocks = [tiling(h, w, 10, 4, (0, 255)) for w, h in sizes]      # 0 / 255 only: every corner has margin 255 and score 254
    images = [flat, chk, tex, tex, tex, blocks, texture_levels(sizes, 4243), texture_levels(sizes, 4244)]
    occ = np.zeros((8, G), np.uint8)
    occ[2] = 1
    occ[4] = random_occupancy(1, G, 0.3, 9)[0]
    return _case("kinds_128x80", packed_table(sizes), images, (6, 4), occ=occ, score=("strip",) * 3, select="rows", sub_n=5)


# 7. a grid that does not cover the image (176x100, cell size 25: the covering grid is 8 x 4)
def _short_grid(cols, rows):
    return _case(f"grid_{cols}x{rows}_on_176x100", packed_table(S176), _stride_images(), (cols, rows), occ=random_occupancy(8, cols * rows, 0.1, 5),
                 score=("strip",) * 3, select="rows", sub_n=2)


# 8. a level larger than level 0 (two levels; the grid covers level 1 at its scale of 2)
def _larger_level(name, size1, stride1, score, select):
    sizes = [(64, 60), size1]
    images = [texture_levels(sizes, 100 * i + 7) for i in range(8)]
    return _case(name, strided_table(sizes, (64, stride1), mod=64, pitch_align=256), images, grid_of(2 * size1[0], 2 * size1[1]), score=score,
                 select=select, sub_n=2)


BUILDERS = {
    "mixed_180x100": lambda: _mixed("mixed_180x100", 180, 100, 3, ("strip", "pixel", "pixel")),
    "mixed_188x120": lambda: _mixed("mixed_188x120", 188, 120, 4, ("strip", "pixel", "pixel", "strip")),
    "production_752x480": _production,
    **{f"grid_{w}x{h}": functools.partial(_grid_width, w, h) for w, h in GRID_SIZES},
    "stride_packed": lambda: _strided("stride_packed", packed_table(S176), ("strip",) * 3, "rows"),
    # aligned padding: offsets multiples of 4 but not of 64 -> the rows kernel with stride != width
    "stride_aligned_padding": lambda: _strided("stride_aligned_padding", strided_table(S176, (184, 96, 48), first=4, gap=8), ("strip",) * 3, "rows"),
    # one odd stride: level 1 goes per-pixel, select<4> with its byte fetch on a level whose width is a multiple of 4
    "stride_odd": lambda: _strided("stride_odd", strided_table(S176, (176, 91, 44), mod=64), ("strip", "pixel", "strip"), "select4"),
    # one odd offset: strides equal the widths, level 1 starts at 2 mod 4
    "offset_odd": lambda: _strided("offset_odd", strided_table(S176, (176, 88, 44), mod=64, offsets=(None, 17602 + 64, None)), ("strip", "pixel", "strip"), "select4"),
    # the last level's last row ends on the last byte of the pitch (frames back to back)
    "tight_pitch": lambda: _strided("tight_pitch", _tight_table(), ("strip",) * 3, "rows"),
    "ties_176x100": lambda: _ties("ties_176x100", 176, ("strip",) * 3, "rows"),
    "ties_180x100": lambda: _ties("ties_180x100", 180, ("strip", "pixel", "pixel"), "select4"),
    "kinds_128x80": _kinds,
    "grid_7x4_on_176x100": lambda: _short_grid(7, 4),
    "grid_6x4_on_176x100": lambda: _short_grid(6, 4),
    "grid_8x3_on_176x100": lambda: _short_grid(8, 3),
    "larger_pixel_level": lambda: _larger_level("larger_pixel_level", (150, 90), 151, ("strip", "pixel"), "select4"),
    "larger_strip_level": lambda: _larger_level("larger_strip_level", (152, 92), 152, ("strip", "strip"), "rows"),
}
NAMES = list(BUILDERS)
SINGLE_FRAME = ["mixed_180x100", "mixed_188x120", "production_752x480", "ties_176x100", "ties_180x100", "grid_7x4_on_176x100",
                "grid_6x4_on_176x100", "grid_8x3_on_176x100"]          # frame 0 also goes through dsdtm_detect_cells
THRESHOLD_CASES = ["grid_176x100", "mixed_180x100"]                      # 5. threshold equality: rows + select<1>, select<4>


@functools.lru_cache(maxsize=None)
def get(name):
    case = BUILDERS[name]()
    assert case.name == name
    for frame in case.images:
        for img in frame:
            img.setflags(write=False)
    case.occ.setflags(write=False)
    return case
