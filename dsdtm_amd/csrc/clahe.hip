// clahe.hip — the kernels of libdsdtm_amd_clahe.so (include/dsdtm_amd_clahe.h), gfx950, 64-lane wavefronts.
//
//   clahe_luts_kernel     E1-E5 for n frames in ONE launch: blockIdx.y is the frame, blockIdx.x the tile, one workgroup of 256 threads
//                         per (tile, frame). Each of the four wavefronts counts into its own 256-bin histogram in LDS with integer LDS
//                         atomics (integer adds commute: the counts do not depend on the order of arrival). A tile that lies within the
//                         image is read as ALIGNED dwords, a thread unpacking the up to four bytes of its dword that belong to the tile's
//                         row (an aligned dword that holds one byte of the row lies in that byte's page: nothing is read that is not
//                         mapped); a tile that touches the extension of E1 is read byte by byte through reflected indices. Then thread i
//                         owns bin i: it sums the four copies, clips, the workgroup reduces `clipped` (a wavefront butterfly, four
//                         partials through LDS), redistributes, scans the 256 counts inclusively (a wavefront scan, four partials
//                         through LDS), rounds (E5) and stores one byte of the tile's table.
//   clahe_interp_kernel   E6 for n frames in ONE launch: blockIdx.z is the frame, blockIdx.y the BAND — the rows whose unclamped ty1 is
//                         blockIdx.y - 1, so that every row of a workgroup reads the same two rows of tables — and blockIdx.x a column
//                         chunk of 256 pixels times a group of 16 rows of the band. The workgroup stages the tables its chunk can reach
//                         (two table rows of at most 16 tiles: at most 8 KiB) in LDS as dwords; a thread has 4 adjacent pixels (their
//                         tx1, tx2 and xa are computed once, the rows of a wavefront share them): one dword load where the source is
//                         aligned for it, four byte gathers from each of the four tables, E6 in float, one dword store where the
//                         destination is aligned for it; byte accesses otherwise and in the tail of a row. The band's first row is found
//                         with the very float expression of E6, so the host and the device cannot disagree about it.
// No kernel waits for another workgroup, nothing depends on an order of arrival, and the interpolation reads the tables across the
// kernel boundary only. Plain C++ only; the float arithmetic is written with plain operators under `fp contract(off)`.
#include "clahe.h"

namespace dsdtm {

// BORDER_REFLECT_101 of an index at or beyond 0 (the mirror repeated where the extension is longer than the side less one)
__device__ __forceinline__ int reflect101(int p, int len) {
    while ((unsigned)p >= (unsigned)len) p = p < 0 ? -p : 2 * (len - 1) - p;
    return p;
}

// saturate_u8(cvRound(v)): halves to even
__device__ __forceinline__ uint32_t round_u8(float v) {
    const float r = rintf(v);
    return r <= 0.0f ? 0u : r >= 255.0f ? 255u : (uint32_t)(int)r;
}

__global__ __launch_bounds__(CLAHE_THREADS) void clahe_luts_kernel(const ClaheFrameDev* __restrict__ frames) {
#pragma clang fp contract(off)
    const ClaheFrameDev f = frames[blockIdx.y];          // (uniform: a copy in scalar registers)
    const int tile = (int)blockIdx.x;
    if (tile >= f.tiles_x * f.tiles_y) return;
    __shared__ int hist[4][256];
    __shared__ int part_clip[4], part_scan[4];
    const int t = (int)threadIdx.x, wave = t >> 6, lane = t & 63;
#pragma unroll
    for (int k = 0; k < 4; ++k) hist[k][t] = 0;
    __syncthreads();
    const int ty = tile / f.tiles_x, tx = tile - ty * f.tiles_x;
    const int x0 = tx * f.tile_w, y0 = ty * f.tile_h;
    int* mine = hist[wave];
    if (x0 + f.tile_w <= f.w && y0 + f.tile_h <= f.h) {
        // E3 within the image. A row of tile_w bytes from any byte offset lies in at most (tile_w + 6) / 4 aligned dwords; the items
        // (row, dword) are dealt to the 256 threads in turn, a thread stepping its pair by 256 items without dividing again.
        const int ndw = (f.tile_w + 6) >> 2;
        int r = t / ndw, j = t - r * ndw;
        const int dr = CLAHE_THREADS / ndw, dj = CLAHE_THREADS - dr * ndw;
        while (r < f.tile_h) {
            const uint8_t* row = f.src + (size_t)(y0 + r) * (size_t)f.src_stride + (size_t)x0;
            const int first = 4 * j - (int)((uintptr_t)row & 3);          // the tile column of the dword's byte 0: -3 .. ; row + first is aligned
            if (first < f.tile_w) {                                        // (first + 3 >= 0: the dword holds a byte of the row)
                const uint32_t v = *reinterpret_cast<const uint32_t*>(row + first);
#pragma unroll
                for (int b = 0; b < 4; ++b)
                    if ((unsigned)(first + b) < (unsigned)f.tile_w) atomicAdd(&mine[(v >> (8 * b)) & 255u], 1);
            }
            r += dr; j += dj;
            if (j >= ndw) { j -= ndw; ++r; }
        }
    } else {
        // E3 on the extension of E1: byte by byte through reflected indices
        int r = t / f.tile_w, c = t - r * f.tile_w;
        const int dr = CLAHE_THREADS / f.tile_w, dc = CLAHE_THREADS - dr * f.tile_w;
        while (r < f.tile_h) {
            const int x = reflect101(x0 + c, f.w), y = reflect101(y0 + r, f.h);
            atomicAdd(&mine[f.src[(size_t)y * (size_t)f.src_stride + (size_t)x]], 1);
            r += dr; c += dc;
            if (c >= f.tile_w) { c -= f.tile_w; ++r; }
        }
    }
    __syncthreads();
    int h = hist[0][t] + hist[1][t] + hist[2][t] + hist[3][t];
    // E4
    int excess = 0;
    if (f.clip > 0 && h > f.clip) { excess = h - f.clip; h = f.clip; }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) excess += __shfl_xor(excess, o, 64);
    if (lane == 0) part_clip[wave] = excess;
    __syncthreads();
    const int clipped = part_clip[0] + part_clip[1] + part_clip[2] + part_clip[3];
    h += (clipped >> 8) + (t < (clipped & 255) ? 1 : 0);
    // E5: the inclusive sum of the 256 counts
    int s = h;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int up = __shfl_up(s, o, 64);
        if (lane >= o) s += up;
    }
    if (lane == 63) part_scan[wave] = s;
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 3; ++k) if (k < wave) s += part_scan[k];
    f.luts[(size_t)tile * 256 + (size_t)t] = (uint8_t)round_u8((float)s * f.scale);
}

// E6 along one axis: floor(p * inv - 0.5f) and the weight of the second table
__device__ __forceinline__ int axis_floor(int p, float inv, float& a) {
#pragma clang fp contract(off)
    const float v = (float)p * inv - 0.5f;
    const float fl = floorf(v);
    a = v - fl;
    return (int)fl;
}

// the first of `len` positions whose axis_floor is at least k (len: none)
__device__ __forceinline__ int first_at_least(int k, int tile, float inv, int len) {
    float a;
    int p = min(max(((2 * k + 1) * tile + 1) / 2, 0), len);          // ceil((k + 0.5) * tile): where it is without rounding
    while (p < len && axis_floor(p, inv, a) < k) ++p;
    while (p > 0 && axis_floor(p - 1, inv, a) >= k) --p;
    return p;
}

__global__ __launch_bounds__(CLAHE_THREADS) void clahe_interp_kernel(const ClaheFrameDev* __restrict__ frames, int subs) {
#pragma clang fp contract(off)
    const ClaheFrameDev f = frames[blockIdx.z];          // (uniform)
    const int band = (int)blockIdx.y;
    const int chunk = (int)blockIdx.x / subs, sub = (int)blockIdx.x - chunk * subs;
    const int xb = chunk * CLAHE_CHUNK;
    if (!f.dst || band > f.tiles_y || xb >= f.w) return;
    // the band: the rows whose unclamped ty1 is band - 1
    const int ys = band == 0 ? 0 : first_at_least(band - 1, f.tile_h, f.inv_th, f.h);
    const int ye = band == f.tiles_y ? f.h : first_at_least(band, f.tile_h, f.inv_th, f.h);
    if (ys + sub * CLAHE_ROWS >= ye) return;
    const int ty1 = min(max(band - 1, 0), f.tiles_y - 1), ty2 = min(band, f.tiles_y - 1);
    // the tables the chunk's columns can reach: tiles txlo .. txhi of the two table rows
    const int xe = min(xb + CLAHE_CHUNK, f.w);
    float unused;
    const int txlo = min(max(axis_floor(xb, f.inv_tw, unused), 0), f.tiles_x - 1);
    const int txhi = min(max(axis_floor(xe - 1, f.inv_tw, unused) + 1, 0), f.tiles_x - 1);
    const int ntx = txhi - txlo + 1;                                        // 1 .. 16
    __shared__ uint32_t staged[2 * DSDTM_CLAHE_MAX_TILES * 64];              // [2][ntx][256 bytes]
    const int t = (int)threadIdx.x, wave = t >> 6, lane = t & 63;
    {
        const uint32_t* g1 = reinterpret_cast<const uint32_t*>(f.luts + ((size_t)ty1 * (size_t)f.tiles_x + (size_t)txlo) * 256);
        const uint32_t* g2 = reinterpret_cast<const uint32_t*>(f.luts + ((size_t)ty2 * (size_t)f.tiles_x + (size_t)txlo) * 256);
        const int nd = ntx * 64;
        for (int i = t; i < nd; i += CLAHE_THREADS) { staged[i] = g1[i]; staged[nd + i] = g2[i]; }
    }
    __syncthreads();
    const int x = xb + lane * CLAHE_PX;
    if (x >= f.w) return;
    const int npx = min((int)CLAHE_PX, f.w - x);
    const uint8_t* l1 = reinterpret_cast<const uint8_t*>(staged);
    const uint8_t* l2 = l1 + ntx * 256;
    int o1[CLAHE_PX], o2[CLAHE_PX];
    float xa[CLAHE_PX];
#pragma unroll
    for (int k = 0; k < CLAHE_PX; ++k) {
        const int i = axis_floor(min(x + k, f.w - 1), f.inv_tw, xa[k]);
        o1[k] = (min(max(i, txlo), txhi) - txlo) * 256;                      // (tx1 = max(i, 0), tx2 = min(i + 1, tiles_x - 1): both within txlo .. txhi)
        o2[k] = (min(max(i + 1, txlo), txhi) - txlo) * 256;
    }
    for (int yb = ys + sub * CLAHE_ROWS; yb < ye; yb += subs * CLAHE_ROWS) {
        const int yend = min(yb + CLAHE_ROWS, ye);
        for (int y = yb + wave; y < yend; y += 4) {
            float ya;
            (void)axis_floor(y, f.inv_th, ya);
            const uint8_t* srow = f.src + (size_t)y * (size_t)f.src_stride + (size_t)x;
            uint32_t v;
            if (npx == CLAHE_PX && ((uintptr_t)srow & 3) == 0) {
                v = *reinterpret_cast<const uint32_t*>(srow);
            } else {
                v = 0;
#pragma unroll
                for (int k = 0; k < CLAHE_PX; ++k) if (k < npx) v |= (uint32_t)srow[k] << (8 * k);
            }
            uint32_t out = 0;
#pragma unroll
            for (int k = 0; k < CLAHE_PX; ++k) {
                const int b = (int)((v >> (8 * k)) & 255u);
                const float a = xa[k];
                const float w11 = (1.0f - a) * (1.0f - ya), w12 = a * (1.0f - ya), w21 = (1.0f - a) * ya, w22 = a * ya;
                float res = (float)l1[o1[k] + b] * w11;
                res = res + (float)l1[o2[k] + b] * w12;
                res = res + (float)l2[o1[k] + b] * w21;
                res = res + (float)l2[o2[k] + b] * w22;
                out |= round_u8(res) << (8 * k);
            }
            uint8_t* drow = f.dst + (size_t)y * (size_t)f.dst_stride + (size_t)x;
            if (npx == CLAHE_PX && ((uintptr_t)drow & 3) == 0) {
                *reinterpret_cast<uint32_t*>(drow) = out;
            } else {
#pragma unroll
                for (int k = 0; k < CLAHE_PX; ++k) if (k < npx) drow[k] = (uint8_t)(out >> (8 * k));
            }
        }
    }
}

hipError_t clahe_luts_launch(const ClaheFrameDev* frames, int n, int max_tiles, hipStream_t stream) {
    if (!frames || n <= 0 || n > DSDTM_CLAHE_MAX_FRAMES || max_tiles <= 0 || max_tiles > DSDTM_CLAHE_MAX_TILES * DSDTM_CLAHE_MAX_TILES) return hipErrorInvalidValue;
    hipLaunchKernelGGL(clahe_luts_kernel, dim3((unsigned)max_tiles, (unsigned)n, 1), dim3(CLAHE_THREADS), 0, stream, frames);
    return hipGetLastError();
}

hipError_t clahe_interp_launch(const ClaheFrameDev* frames, int n, int max_w, int max_tile_h, int max_tiles_y, hipStream_t stream) {
    if (!frames || n <= 0 || n > DSDTM_CLAHE_MAX_FRAMES || max_w <= 0 || max_tile_h <= 0 || max_tiles_y <= 0 || max_tiles_y > DSDTM_CLAHE_MAX_TILES) return hipErrorInvalidValue;
    // groups of 16 rows per band in the grid: at most 16 (a workgroup steps on through a taller band)
    const int subs = (max_tile_h + CLAHE_ROWS - 1) / CLAHE_ROWS < 16 ? (max_tile_h + CLAHE_ROWS - 1) / CLAHE_ROWS : 16;
    const int chunks = (max_w + CLAHE_CHUNK - 1) / CLAHE_CHUNK;
    hipLaunchKernelGGL(clahe_interp_kernel, dim3((unsigned)(chunks * subs), (unsigned)(max_tiles_y + 1), (unsigned)n), dim3(CLAHE_THREADS), 0, stream, frames, subs);
    return hipGetLastError();
}

}  // namespace dsdtm
