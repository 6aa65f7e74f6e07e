// align2d.hip — Feature_Alignment::Align2DGaussNewton, one wavefront per feature (gfx950).
//
// Replaces reference src/Feature_alignment.cpp:318-417. lane = one pixel of the 8x8 patch:
// the lane owns its reference intensity and the gradients derived from the 10x10 bordered
// patch (:330-343) and samples the current image bilinearly each iteration (:381-392). The 3x3
// inverse, the update and the convergence test (:345, :395-411) are evaluated redundantly by all lanes.
// float32 throughout, as the reference (Matrix3f, float u,v) — including its float/double mixing
// in the bilinear weights (:373-376).
//
// The three Jres sums (:389-391) are float sums over the 64 pixels in raster order, and the result
// feeds a threshold (du^2 + dv^2 < 0.03^2, :400) that decides "matched or not" for SearchLocalPoints:
// a differently associated sum can flip that bit for a candidate sitting on the threshold. So the
// sums run in the REFERENCE'S ORDER: every lane parks its products in LDS and three lanes per feature each
// fold one of the sums sequentially (64 dependent float subtractions, the chains side by side;
// align2d_body.h) — pixels and flags are bit-identical to the CPU restatement. (H needs no such care:
// its entries are sums of multiples of 1/4 below 2^22, exact in float in any order.)
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>

#include "kernels.h"
#include "align2d_body.h"

namespace dsdtm {

// SEVERAL features per wavefront — 64 / PPL lanes per feature, PPL pixels of a patch row per lane (PPL = 4, the only shape
// launched: four features per wave, one per 16-lane DPP row; align2d_body.h stays generic in PPL). One wavefront per feature
// (rounds 1-3) carried ONE feature through an iteration's chain — footprint loads -> 64 bilinear samples -> 64 sequential float
// subtractions -> update — with 16 byte gathers per pixel row, and issued the sequential part (which only three lanes need)
// once per feature. Here a wave carries four features through the same chain at once (the reductions of H are group-local DPP
// sums, the 12 sequential Jres chains run side by side), a lane fetches the two footprint rows of its pixels with two wide
// loads, and a launch needs a quarter of the waves. Per pixel the arithmetic is that kernel's, expression for expression; the
// Jres sums run in the reference's raster order (:389-391) as before: pixels and flags stay bit-identical to the CPU
// restatement. Four features per wave: 70 VGPRs, 7 waves per SIMD; eight (114 VGPRs, 4 waves per SIMD) was measured 7 %
// slower — the kernel lives on the waves a compute unit holds.
template <int PPL>
__global__ __launch_bounds__(256) void align2d_rows_kernel(const A2DKernelArgs a) {
    // no FMA contraction: the reference build has none (CMakeLists.txt:5-8, SSE only) and the
    // 0.03^2 convergence threshold (:400) is compared on float values
#pragma clang fp contract(off)
    constexpr int LPF = 64 / PPL;                  // lanes per feature
    constexpr int FPW = 64 / LPF;                  // features per wave
    constexpr int FPB = 4 * FPW;                   // features per 256-thread group
    __shared__ __attribute__((aligned(16))) float s_prod[FPB][192];     // per feature: 3 x 64 products (Jres chains)
    __shared__ LevelGeom s_lv[DSDTM_MAX_LEVELS];
    if (threadIdx.x < DSDTM_MAX_LEVELS) s_lv[threadIdx.x] = a.lv[threadIdx.x];
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const int grp = lane / LPF, l = lane % LPF;                         // feature of the wave, lane of the feature
    const int slot = (threadIdx.x >> 6) * FPW + grp;                    // feature of the workgroup
    const int f = blockIdx.x * FPB + slot;
    float* const prod = s_prod[slot];
    const bool exists = f < a.m;
    const int lvl = exists ? a.level[f] : -1;
    const int fr = (exists && a.frame) ? a.frame[f] : 0;
    const bool valid = exists && !(lvl < 0 || lvl >= a.levels || fr < 0 || (a.frame && fr >= a.n_frames));
    if (exists && !valid && l == 0) a.converged[f] = 0;                 // invalid level / frame: report "not converged"
    const LevelGeom lg = s_lv[valid ? lvl : 0];
    const uint8_t* __restrict__ img = a.cur_pyr + (size_t)fr * a.pyr_pitch + lg.off;
    const int img_size = lg.stride * lg.h;

    const double lscale = (a.px_level0 && valid) ? (double)(1 << lvl) : 1.0;
    float u, v;
    bool converged;
    align2d_rows_feature<PPL>(valid, img, lg, img_size, a.patch_border + (size_t)(valid ? f : 0) * 100, a.patch + (size_t)(valid ? f : 0) * 64, prod,
                              valid ? a.px_xy[2 * (size_t)f] : 0.0, valid ? a.px_xy[2 * (size_t)f + 1] : 0.0, lscale, a.max_iters, lane, u, v, converged);
    if (valid && l == 0) {
        a.px_xy[2 * (size_t)f] = (double)u * lscale;                         // :414 always written back (:154-156 back to level 0)
        a.px_xy[2 * (size_t)f + 1] = (double)v * lscale;
        a.converged[f] = converged ? 1 : 0;
    }
}

hipError_t align2d_launch(const A2DKernelArgs& args, hipStream_t stream) {
    if (args.m <= 0) return hipSuccess;
    hipLaunchKernelGGL(align2d_rows_kernel<4>, dim3((unsigned)((args.m + 15) / 16)), dim3(256), 0, stream, args);
    return hipGetLastError();
}

}  // namespace dsdtm
