// C entries over reject_fundamental_host / check_fundamental_host (dsdtm_amd/host/dsdtm_rarsac_host.hpp) for tests/rarsac_cases.py.
// Test infrastructure only.
#include "../../dsdtm_amd/host/dsdtm_rarsac_host.hpp"

extern "C" int reject_fundamental_host_c(const float* cur, const float* prev, int m, int width, int height, const double* prior, int max_iterations,
                                         double terminate, float sigma, uint32_t seed, uint8_t* status, float* F, double* grid_out, double* score, int* ints) {
    return dsdtm::reject_fundamental_host(cur, prev, m, width, height, prior, max_iterations, terminate, sigma, seed, status, F, grid_out, score, ints);
}

extern "C" int check_fundamental_host_c(const float* cur, const float* prev, int m, int width, int height, const float* F, float sigma, uint8_t* status,
                                        double* grid_out, double* score, int* ints) {
    return dsdtm::check_fundamental_host(cur, prev, m, width, height, F, sigma, status, grid_out, score, ints);
}
