// motion_api.cpp — libdsdtm_amd_motion.so's host side: the one implementation of the models and of a step (motion_api_body.h) under the
// names of include/dsdtm_amd_motion.h.
#define MO_API(name) dsdtm_motion_##name
#define MO_CTX dsdtm_motion_ctx
#define MO_MODEL dsdtm_motion_model
#define MO_LIB "dsdtm_amd_motion"
#include "motion_api_body.h"

extern "C" int dsdtm_motion_steps(dsdtm_motion_ctx* ctx, int n, const dsdtm_motion_desc* descs) {
    std::vector<StepArgs> a;
    if (ctx && descs && n > 0 && n <= DSDTM_MOTION_STEPS_MAX) {
        a.resize((size_t)n);
        for (int t = 0; t < n; ++t) {
            const dsdtm_motion_desc& d = descs[t];
            a[(size_t)t] = StepArgs{d.model, d.image, d.stride, d.mask_stride, d.mask, d.H, d.n_features, d.feature_px, d.feature_on_mask, 0, nullptr};
        }
    }
    return run_steps(ctx, "motion_steps", n, a.empty() ? nullptr : a.data(), false, nullptr);
}

extern "C" int dsdtm_motion_step(dsdtm_motion_ctx* ctx, dsdtm_motion_model* model, const uint8_t* image, int stride, const double* H,
                                 uint8_t* mask, int mask_stride, int n_features, const float* feature_px, uint8_t* feature_on_mask) {
    dsdtm_motion_desc d;
    memset(&d, 0, sizeof d);
    d.model = model; d.image = image; d.stride = stride; d.mask = mask; d.mask_stride = mask_stride; d.H = H;
    d.n_features = n_features; d.feature_px = feature_px; d.feature_on_mask = feature_on_mask;
    return dsdtm_motion_steps(ctx, 1, &d);
}
