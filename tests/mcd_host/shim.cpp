// mcd_box_host (dsdtm_amd/host/dsdtm_mcd_host.hpp) behind a C entry, for tests/mcd_cases.py. Test infrastructure only; it links nothing:
// the header's MotionDetector is never instantiated here.
#include "../../dsdtm_amd/host/dsdtm_mcd_host.hpp"

extern "C" int mcd_box_host_c(const uint8_t* mask, int w, int h, int stride, uint8_t* boxed, int boxed_stride, int32_t* box, int64_t* area2, int32_t* n_components) {
    try {
        const DSDTM::BoxResult r = DSDTM::mcd_box_host(mask, w, h, stride, boxed, boxed_stride);
        for (int k = 0; k < 4; ++k) box[k] = r.box[k];
        *area2 = r.area2; *n_components = r.n_components;
        return 0;
    } catch (...) { return -1; }
}
