"""Cases for dsdtm_pyrdown_batch_device (dsdtm_amd/csrc/pyrdown.hip) in the CALLER's layouts, shared by
tests/test_pyrdown_cases_cpu.py (holds every case to the entry's conditions and to the branch it exists for, with the oracle
alone) and tests/test_pyrdown_gpu.py (runs them on the device).

A case is (name, level-0 width x height, levels, n_images, layout). layout(ws, hs) -> (strides, offsets, pitch, base_shift): the
level table the entry gets, and by how many bytes the first image lies behind the start of the (256-byte aligned) allocation.
build(case) lays the batch out in one host buffer: base_shift bytes, n images of `pitch` bytes, SPARE bytes. Every byte is
POISON but the pixels of level 0 and, around half of level 0's rows, the four bytes before and behind the row where those are
neither pixels nor to be written: 0x00 / 0xFF alternating, so that a padding byte in a filter tap moves a result by more than
rounding. `writable` marks the bytes the call may change: the pixels of levels 1.. and nothing else.

fast_terms() and fused_refusal() restate, as integer arithmetic on the level table, which strips of the per-level kernel take
the 16-byte path and why the one-launch kernel refuses a pyramid. They are no oracle: they classify the cases, so that the CPU
half can assert that every branch has a case, and they keep this table honest against a later edit of a shape.

Nothing here imports the GPU."""
from __future__ import annotations

import ctypes as C
import dataclasses
import functools

import numpy as np

from dsdtm_amd import capi

POISON = 0xA5
SPARE = 256               # bytes behind the last image, inside the allocation


@dataclasses.dataclass(frozen=True)
class Case:
    name: str
    w: int
    h: int
    levels: int
    n: int
    layout: str


def sizes(w, h, levels):
    ws, hs = [], []
    for _ in range(levels):
        ws.append(w); hs.append(h)
        w, h = (w + 1) // 2, (h + 1) // 2
    return ws, hs


def _up(x, m):
    return (x + m - 1) // m * m


# ---- layouts ---------------------------------------------------------------------------------------------------------------
def _packed(ws, hs):
    _, _, ss, offs, total = capi.pyramid_layout(ws[0], hs[0], len(ws))
    return ss, offs, _up(total, 256), 0


def _table(pad, mod=0, shift=0, pitch_mod=0):
    """levels in ascending order: stride = w + pad(l, w); each offset is the first one behind the level before it that is
    mod(l) modulo 16; the pitch is the first size behind the last level that is pitch_mod modulo 16"""
    pad_of = pad if callable(pad) else (lambda l, w: pad)
    mod_of = mod if callable(mod) else (lambda l: mod)

    def layout(ws, hs):
        ss, offs, cur = [], [], 0
        for l, (w, h) in enumerate(zip(ws, hs)):
            s = w + pad_of(l, w)
            o = _up(cur - mod_of(l), 16) + mod_of(l)
            ss.append(s); offs.append(o)
            cur = o + s * h
        return ss, offs, _up(cur - pitch_mod, 16) + pitch_mod, shift
    return layout


def _reversed(ws, hs):
    """levels in descending order of offset, stride == width, level 0 last: its last row ends exactly at the pitch"""
    offs, cur = [0] * len(ws), 0
    for l in range(len(ws) - 1, -1, -1):
        offs[l] = _up(cur, 16)
        cur = offs[l] + ws[l] * hs[l]
    return list(ws), offs, cur, 0


def _mid_last(ws, hs):
    """level 0, levels 2.., then level 1 — a level that is read AND written — ending exactly at the pitch"""
    offs, cur = [0] * len(ws), 0
    for l in [0] + list(range(2, len(ws))) + [1]:
        offs[l] = _up(cur, 16)
        cur = offs[l] + ws[l] * hs[l]
    return list(ws), offs, cur, 0


LAYOUTS = {
    "packed": _packed,                                                   # capi.pyramid_layout: the control
    "padded4": _table(4),                                                # the smallest padding that keeps whole dwords
    "padded12": _table(lambda l, w: 12 if l == 0 else 4),
    "rounded4": _table(lambda l, w: -w % 4),                             # stride = width rounded up to 4: widths 2 mod 4 and odd
    "odd_stride": _table(1),
    "off4": _table(0, mod=4, shift=4),                                   # every level 8 mod 16 in memory: dwords, never 16 bytes
    "off1": _table(0, mod=1),
    "reversed": _reversed,
    "mid_last": _mid_last,
    # one term of the strip's `fast` predicate at a time (2 levels)
    "stride2_l0": _table(lambda l, w: 2 if l == 0 else 0),
    "stride2_l1": _table(lambda l, w: 2 if l == 1 else 0),
    "off1_l0": _table(0, mod=lambda l: 1 if l == 0 else 0),
    "off1_l1": _table(0, mod=lambda l: 1 if l == 1 else 0),
    "pitch2": _table(0, pitch_mod=2),                                    # images 1, 3, .. start at 2 modulo 4
}


# ---- the cases -------------------------------------------------------------------------------------------------------------
def _cases():
    out, ns = [], (1, 3, 5, 9)

    def add(w, h, levels, layout, n=None):
        out.append(Case(f"{w}x{h}_L{levels}_{layout}", w, h, levels, ns[len(out) % 4] if n is None else n, layout))

    # source widths by the last strip: 16 / 24 right strip on the 16-byte path (column sw mirrored), 18 an interior strip that
    # loads columns sw, sw + 1 and a byte-wise last strip of 1 column, 20 / 22 / 30 byte-wise last strips of 2 / 3 / 3 columns
    # (30: behind two 16-byte strips). Heights 9 and 12: chunks of 4 output rows: 5 = 4 + 1 and 6 = 4 + 2 rows, odd and even.
    for w in (16, 18, 20, 22, 24, 30):
        for h in (9, 12):
            add(w, h, 2, "packed")                                       # a stride 2 mod 4 on either level: byte-wise throughout
    for w in (18, 20, 22, 30):                                           # (20: its packed level 1 has a stride of 10)
        for h in (9, 12):
            add(w, h, 2, "rounded4")                                     # ... and with whole dwords per row: the 16-byte path
    for w in (16, 20, 24):
        add(w, 9, 2, "padded4")
        add(w, 12, 2, "padded12")
    # lanes of both paths in one level, over more than one wave (80 and 81 strips); 159-, 161-, 317- and 321-wide levels
    for (w, h), n in (((636, 38), 5), ((642, 21), 3), ((634, 10), 9)):
        add(w, h, 3, "packed", n)
        add(w, h, 3, "rounded4", n)
    # heights below 4 on an otherwise 16-byte shape (general reflection), 4 and 5: the first with one reflection per end
    for h in (1, 2, 3, 4, 5):
        for w in (16, 24):
            add(w, h, 2, "packed")
    for w, h in ((1, 1), (1, 5), (5, 1), (2, 2), (2, 7)):
        add(w, h, 2, "packed")
    # shapes the one-launch kernel takes
    for layout in ("packed", "padded4", "off4"):
        add(64, 37, 3, layout)
        add(128, 64, 5, layout)
    add(64, 37, 3, "padded12")
    add(128, 288, 5, "packed", 32)                                       # pyrdown_fused_kernel<4> with 256 threads in the release library
    for layout in ("odd_stride", "off1"):
        add(16, 9, 2, layout)
        add(24, 12, 2, layout)
        add(64, 37, 3, layout)
    add(16, 9, 2, "off4")
    add(24, 12, 2, "off4")
    # a source level that ends at the pitch
    for w, h, levels in ((16, 9, 2), (24, 12, 2), (20, 12, 2), (64, 37, 3), (128, 64, 5)):
        add(w, h, levels, "reversed")
    add(64, 37, 3, "mid_last", 3)
    # one term of `fast` false, the others true
    for layout in ("stride2_l0", "stride2_l1", "off1_l0", "off1_l1"):
        add(16, 9, 2, layout)
    add(17, 9, 2, "rounded4")
    add(14, 9, 2, "rounded4")
    add(23, 9, 2, "rounded4")                                            # the right-edge rule alone is false only at an odd width
    # refused by the one-launch kernel: image base, width (20 is no multiple of 8), height (3 rows in a source level)
    add(64, 37, 3, "pitch2", 3)
    add(40, 20, 3, "packed")
    add(64, 6, 3, "packed")
    return out


CASES = {c.name: c for c in _cases()}
NAMES = list(CASES)
FUSED_256x4 = "128x288_L5_packed"


# ---- the buffer ------------------------------------------------------------------------------------------------------------
@dataclasses.dataclass
class Built:
    case: Case
    ws: list
    hs: list
    strides: list
    offs: list
    pitch: int
    base_shift: int
    images: list              # n level-0 images (h, w) uint8
    host: np.ndarray          # base_shift + n * pitch + SPARE bytes
    writable: np.ndarray      # bool, same size: the bytes the call may change
    level0: np.ndarray        # bool: the pixels of level 0

    def level(self, buf, i, l):
        """level l of image i inside `buf` (a buffer of host's size) as a strided (h, w) view"""
        o = self.base_shift + i * self.pitch + self.offs[l]
        return np.lib.stride_tricks.as_strided(buf[o:], (self.hs[l], self.ws[l]), (self.strides[l], 1))


def _images(case):
    rng = np.random.default_rng(sum(map(ord, case.name)))
    imgs = [rng.integers(0, 256, (case.h, case.w), dtype=np.uint8) for _ in range(case.n)]
    if case.n >= 2:
        imgs[-1][:] = 255                                                # saturation: (sum + 128) >> 8 stays 255
    if case.n >= 3:
        imp = np.zeros((case.h, case.w), np.uint8)                       # one 255 in each corner and at the centre
        for y in (0, case.h // 2, case.h - 1):
            for x in (0, case.w // 2, case.w - 1):
                if (y == case.h // 2) == (x == case.w // 2):
                    imp[y, x] = 255
        imgs[-2] = imp
    return imgs


@functools.lru_cache(maxsize=None)
def build(name):
    case = CASES[name]
    ws, hs = sizes(case.w, case.h, case.levels)
    ss, offs, pitch, shift = LAYOUTS[case.layout](ws, hs)
    b = Built(case, ws, hs, list(ss), list(offs), pitch, shift, _images(case), None, None, None)
    size = shift + case.n * pitch + SPARE
    b.host = np.full(size, POISON, np.uint8)
    b.writable = np.zeros(size, bool)
    b.level0 = np.zeros(size, bool)
    for i in range(case.n):
        b.level(b.level0, i, 0)[...] = True
        for l in range(1, case.levels):
            b.level(b.writable, i, l)[...] = True
    guard = np.zeros(size, np.int16)                                     # 1: 0x00, 2: 0xFF
    for i in range(case.n):
        for y in range(0, case.h, 2):
            row = shift + i * pitch + offs[0] + y * ss[0]
            for lo, hi in ((row - 4, row), (row + case.w, row + case.w + 4)):
                guard[max(lo, 0):hi] = 1 + (y // 2) % 2
    free = ~b.level0 & ~b.writable
    b.host[free & (guard == 1)] = 0x00
    b.host[free & (guard == 2)] = 0xFF
    for i in range(case.n):
        b.level(b.host, i, 0)[...] = b.images[i]
    for a in (b.host, b.writable, b.level0, *b.images):
        a.setflags(write=False)
    return b


def table_is_valid(b):
    """what the entry asks of a level table — and no two levels of an image share a byte"""
    for l in range(b.case.levels):
        if b.ws[l] <= 0 or b.hs[l] <= 0 or b.strides[l] < b.ws[l] or b.offs[l] + b.strides[l] * b.hs[l] > b.pitch:
            return False
        if l > 0 and (b.ws[l], b.hs[l]) != ((b.ws[l - 1] + 1) // 2, (b.hs[l - 1] + 1) // 2):
            return False
    used = np.zeros(b.pitch, np.int32)
    for l in range(b.case.levels):
        np.lib.stride_tricks.as_strided(used[b.offs[l]:], (b.hs[l], b.ws[l]), (b.strides[l] * 4, 4))[...] += 1
    return used.max() == 1


# ---- the oracle's chain ----------------------------------------------------------------------------------------------------
def oracle_pyrdown_strided(oracle, src, dst):
    """oracle_pyrdown from one strided (h, w) view into another, with the views' own row strides: no copy in between"""
    assert src.strides[1] == 1 and dst.strides[1] == 1 and dst.shape == ((src.shape[0] + 1) // 2, (src.shape[1] + 1) // 2)
    oracle.load().oracle_pyrdown(C.cast(src.ctypes.data, capi.u8p), src.shape[1], src.shape[0], src.strides[0],
                                 C.cast(dst.ctypes.data, capi.u8p), dst.strides[0])


_EXPECTED = {}


def expected(oracle, name):
    """the whole buffer as it must be after the call: the host buffer with levels 1.. of every image filled in by the oracle's
    chain, level by level IN PLACE (strided source, strided destination). Computed once per session; read-only."""
    if name not in _EXPECTED:
        b = build(name)
        buf = b.host.copy()
        for i in range(b.case.n):
            for l in range(1, b.case.levels):
                oracle_pyrdown_strided(oracle, b.level(buf, i, l - 1), b.level(buf, i, l))
        buf.setflags(write=False)
        _EXPECTED[name] = buf
    return _EXPECTED[name]


# ---- the kernels' choices, restated ----------------------------------------------------------------------------------------
TERMS = ("sstride & 3", "source alignment", "sw & 1", "sw >= 16", "sh >= 4", "x4 + 3 < dw", "right edge", "destination alignment",
         "dstride & 3")


def fast_terms(b, i, l):
    """per strip of 4 output columns of level l + 1 of image i: the nine terms of the per-level kernel's `fast`, in TERMS' order.
    The allocation is 16-byte aligned, so an address modulo 4 is its distance from the allocation's start modulo 4."""
    sw, sh, ss, ds = b.ws[l], b.hs[l], b.strides[l], b.strides[l + 1]
    dw = (sw + 1) // 2
    src = b.base_shift + i * b.pitch + b.offs[l]
    dst = b.base_shift + i * b.pitch + b.offs[l + 1]
    out = []
    for x4 in range(0, dw, 4):
        right = 2 * x4 + 8 >= sw                                         # the strip's 11th input column is at or behind sw
        out.append((ss % 4 == 0, src % 4 == 0, sw % 2 == 0, sw >= 16, sh >= 4, x4 + 3 < dw, not right or 2 * x4 + 8 == sw,
                    (dst + x4) % 4 == 0, ds % 4 == 0))
    return out


def strip_classes(b):
    """{'fast', 'generic'} per (image, source level): which paths the strips of that launch take"""
    return {(i, l): {"fast" if all(t) else "generic" for t in fast_terms(b, i, l)} for i in range(b.case.n) for l in range(b.case.levels - 1)}


def false_term_sets(b):
    """every set of false terms some strip of the case has"""
    return {frozenset(TERMS[k] for k, ok in enumerate(t) if not ok) for i in range(b.case.n) for l in range(b.case.levels - 1)
            for t in fast_terms(b, i, l)}


def tight(b, l):
    """fewer than 4 bytes inside the pitch behind the last row of level l, and fewer than 4 bytes of row padding"""
    return b.strides[l] < b.ws[l] + 4 and b.pitch - (b.offs[l] + b.strides[l] * b.hs[l]) < 4


def fused_refusal(b):
    """None if the one-launch kernel takes the pyramid, else the first reason it does not, in the launcher's order"""
    L = b.case.levels
    if L < 3 or L > 5:
        return "levels"
    if b.base_shift % 4 or b.pitch % 4:
        return "base or pitch"
    for l in range(L):
        if b.strides[l] % 4 or b.offs[l] % 4:
            return "stride or offset"
        if l < L - 1 and (b.ws[l] % 8 or b.ws[l] < 16):
            return "width"
        if b.hs[l] < (4 if l < L - 1 else 1):
            return "height"
    if tight(b, 0):
        return "level 0 ends at the pitch"
    return None


def fused_plan(b, band=0):
    """(band, bands, bytes of LDS) of the one-launch kernel for an eligible pyramid, by the launcher's band rule"""
    K, n, hs, ws = b.case.levels - 1, b.case.n, b.hs, b.ws
    if band <= 0:
        nb = max(4, -(-2048 // n))
        band = max(-(-hs[K] // nb), 1 if n * hs[K] <= 256 else 2)
    band = min(band, hs[K])
    while True:
        bands, lds = -(-hs[K] // band), 0
        for l in range(1, K):
            rows = 0
            for k in range(bands):
                lo, hi = k * band, min(k * band + band, hs[K])
                for m in range(K - 1, l - 1, -1):
                    lo, hi = max(2 * lo - 2, 0), min(2 * hi + 1, hs[m])
                rows = max(rows, hi - lo)
            lds += _up(rows * ws[l] + 16, 16)
        if lds <= 64 * 1024 or band <= 2:
            return band, bands, lds
        band = (band + 1) // 2


def release_kernel(b):
    """the kernel the release library picks: 'per level', or (K, threads) of the one-launch kernel"""
    if b.case.n > 32 or fused_refusal(b) is not None:
        return "per level"
    band, bands, lds = fused_plan(b)
    if lds > 64 * 1024:
        return "per level"
    K = b.case.levels - 1
    return (K, 1024) if K == 4 and bands * b.case.n <= 256 else (K, 256)
