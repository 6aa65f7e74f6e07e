// contour.hip — the contour step of MCDWrapper::Run (Thirdparty/fastMCD/src/MCDWrapper.cpp:98-128) for n masks on gfx950: rules C1-C5 of
// include/dsdtm_amd_mcd.h. Integer only; every result is a function of the mask, not of the order in which threads arrive.
//
//   label    a pixel's label is its own index (foreground) or -1
//   merge    union-find over the 8-neighbourhood: a foreground pixel joins its W / NW / N / NE neighbours by atomicMin on the larger root,
//            so a component's root is its lowest pixel index = its raster-first pixel (C2's start). Labels only ever fall and always
//            name a pixel of the same component, so a value another workgroup has since lowered still leads to the root; every access
//            in this launch is an agent-scope atomic, and what the launch leaves is read by the launches behind it.
//   flatten  label = root; at the root the component's extents by atomicMin / atomicMax (only pixels that have no neighbour of their
//            component further out take part), the roots appended to a list (atomicAdd: the list's ORDER is arrival order, its CONTENT
//            is not, and nothing below depends on the order)
//   trace    one workgroup per mask: the bit-plane into LDS, a sort key per root (the bound 2 (bw - 1)(bh - 1) on area2, then the lowest
//            root), then round by round the largest key below the last one; thread 0 walks that component's outer border (C2) and sums
//            area2 (C3). The rounds end when the bound falls below the best area2, or equals it at a higher root (C4's tie rule).
//   fill     C5, behind it.
#include "contour.h"

namespace dsdtm {
namespace {

constexpr int LABEL_THREADS = 256;

__device__ __forceinline__ int32_t ld(const int32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// (labels fall strictly along a chain: the walk ends at the first entry that does not point lower, whatever it reads)
__device__ __forceinline__ int32_t find_root(const int32_t* L, int32_t x) {
    for (;;) {
        const int32_t p = ld(L + x);
        if (p < 0 || p >= x) return x;
        x = p;
    }
}

// joins the components of pixels a and b: the larger root is pointed at the smaller one; where another thread got there first the
// union goes on from what it left (a falls with every turn)
__device__ void unite(int32_t* L, int32_t a, int32_t b) {
    for (;;) {
        a = find_root(L, a);
        b = find_root(L, b);
        if (a == b) return;
        if (a < b) { const int32_t t = a; a = b; b = t; }
        const int32_t old = __hip_atomic_fetch_min(L + a, b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (old == a) return;
        a = old;
    }
}

__device__ __forceinline__ int padded(int pixels) { return (pixels + 3) / 4 * 4; }      // contour_bind_scratch's

__global__ __launch_bounds__(LABEL_THREADS) void contour_label_kernel(const ContourDev* __restrict__ recs) {
    const ContourDev r = recs[blockIdx.y];
    const int pixels = r.width * r.height, px = padded(pixels);
    const int p = (int)blockIdx.x * LABEL_THREADS + (int)threadIdx.x;
    if (p == 0) { ContourResult z = {{0, 0, 0, 0}, 0, 0, 0}; *r.result = z; }
    if (p >= pixels) return;
    const int y = p / r.width, x = p - y * r.width;
    r.label[p] = r.src[(size_t)y * (size_t)r.src_pitch + (size_t)x] != 0 ? p : -1;        // C1
    r.ext[p] = 0x7FFFFFFF;
    r.ext[px + p] = -1;
    r.ext[2 * px + p] = -1;
}

__global__ __launch_bounds__(LABEL_THREADS) void contour_merge_kernel(const ContourDev* __restrict__ recs) {
    const ContourDev r = recs[blockIdx.y];
    const int w = r.width, pixels = w * r.height;
    const int p = (int)blockIdx.x * LABEL_THREADS + (int)threadIdx.x;
    if (p >= pixels || ld(r.label + p) < 0) return;
    const int y = p / w, x = p - y * w;
    // (N joins NW and NE to this pixel by their own W links)
    if (y > 0 && ld(r.label + p - w) >= 0) unite(r.label, p, p - w);
    else if (y > 0) {
        if (x > 0 && ld(r.label + p - w - 1) >= 0) unite(r.label, p, p - w - 1);
        if (x < w - 1 && ld(r.label + p - w + 1) >= 0) unite(r.label, p, p - w + 1);
    }
    if (x > 0 && ld(r.label + p - 1) >= 0) unite(r.label, p, p - 1);
}

__global__ __launch_bounds__(LABEL_THREADS) void contour_flatten_kernel(const ContourDev* __restrict__ recs) {
    const ContourDev r = recs[blockIdx.y];
    const int w = r.width, h = r.height, pixels = w * h, px = padded(pixels);
    const int p = (int)blockIdx.x * LABEL_THREADS + (int)threadIdx.x;
    if (p >= pixels || ld(r.label + p) < 0) return;
    const int32_t root = find_root(r.label, p);
    __hip_atomic_store(r.label + p, root, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const int y = p / w, x = p - y * w;
    auto on = [&](int q) { return ld(r.label + q) >= 0; };
    if (!(x > 0 && on(p - 1))) atomicMin(r.ext + root, x);
    if (!(x < w - 1 && on(p + 1))) atomicMax(r.ext + px + root, x);
    if (!(y < h - 1 && (on(p + w) || (x > 0 && on(p + w - 1)) || (x < w - 1 && on(p + w + 1))))) atomicMax(r.ext + 2 * px + root, y);
    if (root == p) {
        const int slot = atomicAdd(&r.result->n_components, 1);
        if ((size_t)slot < contour_list_cap(w, h)) r.roots[slot] = (uint32_t)p;
    }
}

__device__ __forceinline__ unsigned long long wave_max_u64(unsigned long long v) {
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned long long o = __shfl_xor(v, off, 64);
        v = o > v ? o : v;
    }
    return v;
}

// directions as OpenCV's border follower numbers them: 0 = E, then counter-clockwise on the screen (1 = NE, 2 = N, ... 7 = SE)
__device__ __forceinline__ int dir_dx(int s) { return (int)(0x901Au >> (2 * s) & 3u) - 1; }      // 1, 1, 0, -1, -1, -1, 0, 1
__device__ __forceinline__ int dir_dy(int s) { return (int)(0xA901u >> (2 * s) & 3u) - 1; }      // 0, -1, -1, -1, 0, 1, 1, 1

__global__ __launch_bounds__(CONTOUR_TRACE_THREADS) void contour_trace_kernel(const ContourDev* __restrict__ recs) {
    extern __shared__ uint32_t bits[];
    __shared__ unsigned long long red[CONTOUR_TRACE_THREADS / 64];
    __shared__ long long s_area2;
    __shared__ int s_status;
    const ContourDev r = recs[blockIdx.x];
    const int tid = (int)threadIdx.x, w = r.width, h = r.height;
    // (the host checked the size; it bounds the LDS array, so it is clamped here once more)
    const int pixels = min(w * h, CONTOUR_MAX_PIXELS), px = padded(w * h), words = (pixels + 31) >> 5;
    for (int base = 0; base < words * 32; base += CONTOUR_TRACE_THREADS) {
        const int p = base + tid;
        const unsigned long long b = __ballot(p < pixels && r.label[p] >= 0);
        if ((tid & 63) == 0) {
            const int wi = p >> 5;
            if (wi < words) bits[wi] = (uint32_t)b;
            if (wi + 1 < words) bits[wi + 1] = (uint32_t)(b >> 32);
        }
    }
    const int found = r.result->n_components, cap = (int)contour_list_cap(w, h);
    const int m = found < 0 ? 0 : found < cap ? found : cap;
    for (int i = tid; i < m; i += CONTOUR_TRACE_THREADS) {
        const uint32_t root = r.roots[i];
        unsigned long long key = 0;
        if (root < (uint32_t)pixels) {
            const long long bw = (long long)r.ext[px + root] - r.ext[root], bh = (long long)r.ext[2 * px + root] - (int)(root / (uint32_t)w);
            if (bw > 0 && bh > 0 && bw < 4096 && bh < 4096) key = (unsigned long long)(2 * bw * bh) << 32 | (0xFFFFFFFFu - root);
        }
        r.keys[i] = key;          // 0: a dot or a line (area2 = 0 <= any bound), never visited
    }
    if (tid == 0) s_status = 0;
    __syncthreads();

    auto on = [&](int x, int y) -> bool {
        if ((unsigned)x >= (unsigned)w || (unsigned)y >= (unsigned)h) return false;
        const int p = y * w + x;
        return p < pixels && (bits[p >> 5] >> (p & 31) & 1u);
    };
    unsigned long long cursor = ~0ull, best = 0;
    uint32_t best_root = 0xFFFFFFFFu;
    for (int round = 0; round < m; ++round) {
        unsigned long long top = 0;
        for (int i = tid; i < m; i += CONTOUR_TRACE_THREADS) {
            const unsigned long long k = r.keys[i];
            if (k < cursor && k > top) top = k;
        }
        top = wave_max_u64(top);
        if ((tid & 63) == 0) red[tid >> 6] = top;
        __syncthreads();
        top = 0;
        for (int k = 0; k < CONTOUR_TRACE_THREADS / 64; ++k) top = red[k] > top ? red[k] : top;
        if (top == 0) break;
        const unsigned long long bound = top >> 32;
        const uint32_t root = 0xFFFFFFFFu - (uint32_t)top;
        if (bound < best || (bound == best && root > best_root)) break;
        if (tid == 0) {
            // C2: the outer border from the raster-first pixel, entered from its left neighbour
            const int x0 = (int)(root % (uint32_t)w), y0 = (int)(root / (uint32_t)w);
            long long acc = 0;
            int s = 4;
            do { s = (s - 1) & 7; } while (!on(x0 + dir_dx(s), y0 + dir_dy(s)) && s != 4);
            if (s != 4) {
                const int x1 = x0 + dir_dx(s), y1 = y0 + dir_dy(s);
                int x = x0, y = y0, left = 4 * pixels + 4;
                for (;;) {
                    if (--left < 0) { s_status = 1; acc = 0; break; }
                    unsigned nb = 0;
#pragma unroll
                    for (int k = 0; k < 8; ++k) nb |= (unsigned)on(x + dir_dx(k), y + dir_dy(k)) << k;
                    if (nb == 0) { s_status = 1; acc = 0; break; }          // (the pixel it came from is set: cannot happen)
                    const unsigned rot = ((nb | nb << 8) >> (s + 1)) & 0xFFu;       // the first set neighbour counter-clockwise behind s
                    s = (s + 1 + __builtin_ctz(rot)) & 7;
                    const int nx = x + dir_dx(s), ny = y + dir_dy(s);
                    acc += (long long)x * ny - (long long)y * nx;              // C3
                    if (nx == x0 && ny == y0 && x == x1 && y == y1) break;      // Suzuki's stop: about to repeat the first move
                    x = nx; y = ny; s = (s + 4) & 7;
                }
            }
            s_area2 = acc < 0 ? -acc : acc;
        }
        __syncthreads();
        const unsigned long long a2 = (unsigned long long)s_area2;
        if (a2 > best || (a2 == best && a2 > 0 && root < best_root)) { best = a2; best_root = root; }      // C4
        cursor = top;
    }
    __syncthreads();
    if (tid == 0) {
        ContourResult out = {{0, 0, 0, 0}, 0, r.result->n_components, s_status};
        if (best > 0 && s_status == 0 && best_root < (uint32_t)pixels) {
            const int minx = r.ext[best_root], miny = (int)(best_root / (uint32_t)w);
            out.box[0] = minx; out.box[1] = miny;
            out.box[2] = r.ext[px + best_root] - minx + 1; out.box[3] = r.ext[2 * px + best_root] - miny + 1;
            out.area2 = (long long)best;
        }
        *r.result = out;
    }
}

__global__ __launch_bounds__(LABEL_THREADS) void contour_fill_kernel(const ContourDev* __restrict__ recs) {
    const ContourDev r = recs[blockIdx.y];
    const int p = (int)blockIdx.x * LABEL_THREADS + (int)threadIdx.x;
    if (!r.dst || p >= r.width * r.height) return;
    const int y = p / r.width, x = p - y * r.width;
    const int bx = r.result->box[0], by = r.result->box[1], bw = r.result->box[2], bh = r.result->box[3];
    uint8_t* at = r.dst + (size_t)y * (size_t)r.dst_pitch + (size_t)x;
    if (x >= bx && x < bx + bw && y >= by && y < by + bh) *at = 255;             // C5: minx..maxx x miny..maxy inclusive
    else if (r.dst != r.src) *at = r.src[(size_t)y * (size_t)r.src_pitch + (size_t)x];
}

}  // namespace

hipError_t contour_launch(const ContourDev* recs, int n, int max_pixels, hipStream_t stream) {
    if (n <= 0) return hipSuccess;
    if (!recs || max_pixels <= 0 || max_pixels > CONTOUR_MAX_PIXELS) return hipErrorInvalidValue;
    const dim3 grid((unsigned)((max_pixels + LABEL_THREADS - 1) / LABEL_THREADS), (unsigned)n);
    contour_label_kernel<<<grid, LABEL_THREADS, 0, stream>>>(recs);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    contour_merge_kernel<<<grid, LABEL_THREADS, 0, stream>>>(recs);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    contour_flatten_kernel<<<grid, LABEL_THREADS, 0, stream>>>(recs);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    const size_t lds = ((size_t)(max_pixels + 31) / 32 + 2) * 4;
    if (lds > 64 * 1024) {      // more than 64 KB of dynamic LDS is an opt-in per kernel and device; harmless to repeat
        e = hipFuncSetAttribute((const void*)contour_trace_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
    }
    contour_trace_kernel<<<(unsigned)n, CONTOUR_TRACE_THREADS, lds, stream>>>(recs);
    return hipGetLastError();
}

hipError_t contour_fill_launch(const ContourDev* recs, int n, int max_pixels, hipStream_t stream) {
    if (n <= 0) return hipSuccess;
    if (!recs || max_pixels <= 0 || max_pixels > CONTOUR_MAX_PIXELS) return hipErrorInvalidValue;
    contour_fill_kernel<<<dim3((unsigned)((max_pixels + LABEL_THREADS - 1) / LABEL_THREADS), (unsigned)n), LABEL_THREADS, 0, stream>>>(recs);
    return hipGetLastError();
}

}  // namespace dsdtm
