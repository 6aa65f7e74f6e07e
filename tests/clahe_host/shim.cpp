// C entries over clahe_host / clahe_luts_host (dsdtm_amd/host/dsdtm_clahe_host.hpp) for tests/clahe_cases.py.
// Test infrastructure only.
#include "../../dsdtm_amd/host/dsdtm_clahe_host.hpp"

extern "C" void clahe_host_c(const uint8_t* src, int src_stride, uint8_t* dst, int dst_stride, int width, int height, double clip_limit, int tiles_x,
                             int tiles_y, uint8_t* lut_out) {
    DSDTM::clahe_host(src, src_stride, dst, dst_stride, width, height, clip_limit, tiles_x, tiles_y, lut_out);
}

extern "C" void clahe_luts_host_c(const uint8_t* src, int src_stride, int width, int height, double clip_limit, int tiles_x, int tiles_y, uint8_t* luts) {
    DSDTM::clahe_luts_host(src, src_stride, width, height, clip_limit, tiles_x, tiles_y, luts);
}
