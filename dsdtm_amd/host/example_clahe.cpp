// example_clahe.cpp — the first lines of the reference's detector driver (Test/test_Feature_detection.cpp:85-86): a low-contrast frame goes
// through cv::createCLAHE(3.0, cv::Size(8, 8))->apply — here DSDTM::CLAHE (libdsdtm_amd_clahe.so) from pageable host memory into device
// memory — then dsdtm_frame_prefetch on that device pointer (read in place) and dsdtm_detect_cells_frame (libdsdtm_amd.so). The frame is
// generated here: a faint checker texture on a bright ramp, on which FAST at the reference's barrier of 20 finds little; the program prints how many
// cells hold a corner before and after the contrast has been equalised. The device result is held against clahe_host, the same rules on the host.
//   build: g++ -std=c++14 -ffp-contract=off example_clahe.cpp -L../csrc -ldsdtm_amd_clahe -ldsdtm_amd -L/opt/rocm/lib -lamdhip64 -o example_clahe
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "dsdtm_clahe_host.hpp"

// (the HIP runtime calls this program makes itself, declared here so that it needs no HIP header: hipError_t is an int, 0 = hipSuccess;
// hipMemcpy's kind 2 is device to host)
extern "C" int hipMalloc(void** ptr, size_t bytes);
extern "C" int hipFree(void* ptr);
extern "C" int hipMemcpy(void* dst, const void* src, size_t bytes, int kind);

#define HIP_OK(call) do { if ((call) != 0) { std::fprintf(stderr, "%s failed\n", #call); return 1; } } while (0)
#define DSDTM_CHECK(call) do { if ((call) != DSDTM_OK) { std::fprintf(stderr, "%s: %s\n", #call, dsdtm_last_error(ctx)); return 1; } } while (0)

static int count_corners(dsdtm_ctx* ctx, const uint8_t* d_gray, int W, int H, int levels, int* out) {
    dsdtm_frame_image im{};
    im.gray = d_gray; im.width = W; im.height = H; im.stride = W; im.levels = levels;
    dsdtm_frame* frame = nullptr;
    DSDTM_CHECK(dsdtm_frame_prefetch(ctx, &im, &frame));          // returns at once; reads the device buffer in place
    dsdtm_detect_params p{};
    p.cell_size = 25; p.grid_cols = (W + 24) / 25; p.grid_rows = (H + 24) / 25; p.levels = levels; p.barrier = 20; p.detection_threshold = 20.0f;
    const size_t cells = (size_t)p.grid_cols * p.grid_rows;
    std::vector<uint8_t> occupied(cells, 0);
    std::vector<float> score(cells);
    std::vector<int32_t> cx(cells), cy(cells), cl(cells);
    DSDTM_CHECK(dsdtm_detect_cells_frame(ctx, frame, occupied.data(), &p, score.data(), cx.data(), cy.data(), cl.data()));
    *out = 0;
    for (size_t k = 0; k < cells; ++k) *out += score[k] > p.detection_threshold ? 1 : 0;
    dsdtm_frame_destroy(ctx, frame);
    return 0;
}

int main() {
    const int W = 640, H = 480, LEVELS = 3;
    std::vector<uint8_t> raw((size_t)W * H), want((size_t)W * H), got((size_t)W * H);
    for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x) raw[(size_t)y * W + x] = (uint8_t)(150 + x / 16 + (((x / 12) + (y / 12)) % 2 ? 14 : 0));
    dsdtm_ctx* ctx = nullptr;
    if (dsdtm_create(0, &ctx) != DSDTM_OK) { std::fprintf(stderr, "dsdtm_create: %s\n", dsdtm_last_error(nullptr)); return 1; }
    uint8_t* d_raw = nullptr;
    uint8_t* d_eq = nullptr;
    HIP_OK(hipMalloc((void**)&d_raw, raw.size()));
    HIP_OK(hipMalloc((void**)&d_eq, raw.size()));
    int before = 0, after = 0;
    try {
        DSDTM::CLAHE clahe(3.0, 8, 8);                                // the context is made at the first apply and kept
        clahe.apply(DSDTM::GrayImage{raw.data(), W, H, W}, DSDTM::GrayImage{d_eq, W, H, W});      // pageable host -> device; complete on return
    } catch (const std::exception& e) { std::fprintf(stderr, "%s\n", e.what()); return 1; }
    HIP_OK(hipMemcpy(got.data(), d_eq, got.size(), 2));
    DSDTM::clahe_host(raw.data(), W, want.data(), W, W, H);          // the same rules on the host: bit-equal
    HIP_OK(hipMemcpy(d_raw, raw.data(), raw.size(), 1));
    if (count_corners(ctx, d_raw, W, H, LEVELS, &before) || count_corners(ctx, d_eq, W, H, LEVELS, &after)) return 1;
    std::printf("cells with a corner: %d on the raw frame, %d on the equalised frame; device %s host\n", before, after, got == want ? "==" : "!=");
    const bool ok = got == want && after >= before;
    (void)hipFree(d_raw); (void)hipFree(d_eq);
    dsdtm_destroy(ctx);
    std::printf("%s\n", ok ? "ok" : "FAILED");
    return ok ? 0 : 1;
}
