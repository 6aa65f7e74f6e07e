// contour.h — launch-side declarations shared by contour.hip and mcd_api.cpp (libdsdtm_amd_mcd.so): the contour step of MCDWrapper::Run
// (rules C1-C5 of include/dsdtm_amd_mcd.h) on 8-bit masks in device memory.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace dsdtm {

constexpr int CONTOUR_MAX_PIXELS = 1 << 20;                // the bit-plane of one mask must fit one workgroup's LDS (128 KB of 160)
constexpr size_t CONTOUR_SCRATCH_BUDGET = (size_t)1 << 30; // scratch of the masks that go through the kernels together (a batch beyond it runs in turns)
constexpr int CONTOUR_TRACE_THREADS = 1024;

// What a mask's walk leaves (read back as it is): box = x, y, w, h, all 0 when no rectangle is drawn; area2 = twice the winner's area;
// status != 0: a walk passed its cap of 4 * pixels + 4 steps (never, by construction; the host turns it into an error)
struct ContourResult {
    int32_t box[4];
    int64_t area2;
    int32_t n_components;
    int32_t status;
};

// One mask as the kernels see it. label: pixels (a pixel's component = its lowest pixel index; -1 background); ext: 3 x pixels, at a
// component's root its smallest x, largest x and largest y (its smallest y is the root's); roots / keys: list_cap entries, the roots in
// arrival order and their sort keys.
struct ContourDev {
    const uint8_t* src;        // the mask, rows src_pitch apart
    uint8_t* dst;              // where the mask with the rectangle goes (may be src: then only the rectangle is written); NULL: nowhere
    int32_t* label;
    int32_t* ext;
    uint32_t* roots;
    unsigned long long* keys;
    ContourResult* result;
    int32_t width, height, src_pitch, dst_pitch;
};

// 8-connected components are at least one background pixel apart: no more than ceil(w / 2) * ceil(h / 2) of them
constexpr size_t contour_list_cap(int w, int h) { return (size_t)((w + 1) / 2) * (size_t)((h + 1) / 2); }
inline size_t contour_scratch_bytes(int w, int h) {
    const size_t px = ((size_t)w * (size_t)h + 3) / 4 * 4, cap = (contour_list_cap(w, h) + 3) / 4 * 4;
    return px * 16 + cap * 12;
}
inline void contour_bind_scratch(ContourDev& r, uint8_t* base) {      // base: 16-byte aligned device memory of contour_scratch_bytes
    const size_t px = ((size_t)r.width * (size_t)r.height + 3) / 4 * 4, cap = (contour_list_cap(r.width, r.height) + 3) / 4 * 4;
    r.keys = (unsigned long long*)base;
    r.label = (int32_t*)(base + cap * 8);
    r.ext = r.label + px;
    r.roots = (uint32_t*)(r.ext + 3 * px);
}

// C1-C4 for n masks (every width * height <= max_pixels <= CONTOUR_MAX_PIXELS): four launches — labels, merges, flatten + extents, and
// one workgroup per mask that walks the candidates' borders on the bit-plane in LDS and writes the result.
hipError_t contour_launch(const ContourDev* recs, int n, int max_pixels, hipStream_t stream);
// C5 behind it: dst = src with the result's rectangle set to 255 (one launch; records without dst are passed over)
hipError_t contour_fill_launch(const ContourDev* recs, int n, int max_pixels, hipStream_t stream);

}  // namespace dsdtm
