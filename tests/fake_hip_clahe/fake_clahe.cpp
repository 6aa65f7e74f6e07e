// The fakes of the two launch functions of dsdtm_amd/csrc/clahe.hip for the fake HIP runtime of tests/fake_hip, which is used unmodified
// and knows nothing of them. That runtime runs queued operations only when something waits for them, so a fake first drains the stream
// (the upload queued in front of it then runs) and then does the kernel's work with the host functions of
// dsdtm_amd/host/dsdtm_clahe_host.hpp on the very pointers and strides of the records: under AddressSanitizer an offset, a stride or a
// count that leaves its buffer shows up here, and the driver predicts every byte with the same functions. The geometry in a record is
// held against clahe_geometry of the record's sizes (the clip limit cannot be recovered from a record: its `clip` is taken as it is).
// Test infrastructure only.
#include <atomic>
#include <cstdint>
#include <cstring>

#include "fake_hip.h"
#include "fake_clahe.h"
#include "clahe.h"
#include "../../dsdtm_amd/host/dsdtm_clahe_host.hpp"

static std::atomic<long> g_fail{0}, g_launches{0};
void fake_clahe_fail(long nth) { g_fail = nth; }
long fake_clahe_launches() { return g_launches; }

namespace dsdtm {

// the record's geometry as the host functions want it, or false where the record contradicts itself
static bool geometry_of(const ClaheFrameDev& f, DSDTM::ClaheGeometry* g) {
    if (!f.src || !f.luts || ((uintptr_t)f.luts & 255) || f.w < DSDTM_CLAHE_MIN_SIDE || f.h < DSDTM_CLAHE_MIN_SIDE || f.w > DSDTM_CLAHE_MAX_SIDE ||
        f.h > DSDTM_CLAHE_MAX_SIDE || f.src_stride < f.w || f.tiles_x < 1 || f.tiles_y < 1 || f.tiles_x > DSDTM_CLAHE_MAX_TILES || f.tiles_y > DSDTM_CLAHE_MAX_TILES)
        return false;
    *g = DSDTM::clahe_geometry(f.w, f.h, 0.0, f.tiles_x, f.tiles_y);
    if (g->tile_w != f.tile_w || g->tile_h != f.tile_h || g->scale != f.scale || g->inv_tw != f.inv_tw || g->inv_th != f.inv_th || f.clip < 0 || f.clip > g->area)
        return false;
    g->clip = f.clip;
    return true;
}

hipError_t clahe_luts_launch(const ClaheFrameDev* frames, int n, int max_tiles, hipStream_t stream) {
    if (g_fail > 0 && --g_fail == 0) return hipErrorUnknown;
    if (!frames || n <= 0 || n > DSDTM_CLAHE_MAX_FRAMES) return hipErrorInvalidValue;
    if (hipStreamSynchronize(stream) != hipSuccess) return hipErrorUnknown;
    ++g_launches;
    int seen = 0;
    for (int t = 0; t < n; ++t) {
        ClaheFrameDev f;
        memcpy(&f, frames + t, sizeof f);
        DSDTM::ClaheGeometry g;
        if (!geometry_of(f, &g) || g.tiles_x * g.tiles_y > max_tiles) return hipErrorInvalidValue;
        seen = g.tiles_x * g.tiles_y > seen ? g.tiles_x * g.tiles_y : seen;
        // (clahe_luts_host takes a clip LIMIT: the one that gives this record's clip back, or 0)
        const double limit = f.clip == 0 ? 0.0 : ((double)f.clip + 0.5) * 256.0 / (double)g.area;
        if (DSDTM::clahe_geometry(f.w, f.h, limit, f.tiles_x, f.tiles_y).clip != f.clip) return hipErrorInvalidValue;
        DSDTM::clahe_luts_host(f.src, f.src_stride, f.w, f.h, limit, f.tiles_x, f.tiles_y, f.luts);
    }
    return seen == max_tiles ? hipSuccess : hipErrorInvalidValue;      // the grid is sized by the largest frame, no larger
}

hipError_t clahe_interp_launch(const ClaheFrameDev* frames, int n, int max_w, int max_tile_h, int max_tiles_y, hipStream_t stream) {
    if (g_fail > 0 && --g_fail == 0) return hipErrorUnknown;
    if (!frames || n <= 0 || n > DSDTM_CLAHE_MAX_FRAMES) return hipErrorInvalidValue;
    if (hipStreamSynchronize(stream) != hipSuccess) return hipErrorUnknown;
    ++g_launches;
    int seen_w = 0, seen_th = 0, seen_ty = 0;
    for (int t = 0; t < n; ++t) {
        ClaheFrameDev f;
        memcpy(&f, frames + t, sizeof f);
        DSDTM::ClaheGeometry g;
        if (!geometry_of(f, &g) || !f.dst || f.dst_stride < f.w || f.w > max_w || g.tile_h > max_tile_h || g.tiles_y > max_tiles_y) return hipErrorInvalidValue;
        seen_w = f.w > seen_w ? f.w : seen_w; seen_th = g.tile_h > seen_th ? g.tile_h : seen_th; seen_ty = g.tiles_y > seen_ty ? g.tiles_y : seen_ty;
        DSDTM::clahe_interpolate_host(f.src, f.src_stride, f.dst, f.dst_stride, f.w, f.h, g, f.luts);
    }
    return seen_w == max_w && seen_th == max_tile_h && seen_ty == max_tiles_y ? hipSuccess : hipErrorInvalidValue;
}

}  // namespace dsdtm
