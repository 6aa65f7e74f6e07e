// motion.hip — the moving-object mask of fastMCD for n independent models in one launch (libdsdtm_amd_motion.so, gfx950).
//
// What one step is: MCDWrapper::Run (Thirdparty/fastMCD/src/MCDWrapper.cpp:65-137) up to BGModel.update(detect_img) — the 5x5
// median of the image (BORDER_REPLICATE), ProbModel::motionCompensate and the three passes of ProbModel::update
// (Thirdparty/fastMCD/include/prob_model.h:169-371, :373-582). Every cell depends on the OLD m_Mean / m_Var / m_Age of up to four
// cells and on its own _Temp entries, so compensation and all of update are one pass over the cells: read generation `src`, write
// every entry of generation `dst`.
//
// A workgroup of 256 threads owns 16 x 16 cells = 64 x 64 pixels. It brings its pixels with a 2-pixel replicated halo into LDS
// (68 rows of 68 bytes at a pitch of 80), then one thread per cell takes its 8 x 8 window out of LDS as 16 dwords, selects the 16
// medians of 25 in registers (min / max only), and runs compensation and update for its cell. It writes its cell of the new model
// and its 4 x 4 pixels of the mask (one dword per row), nothing else.
// LDS: a thread's window row r starts at dword (4 cy + r) * 20 + cx. ds_read_b32 serves lanes in halves of 32 = two cell rows
// (cy, cy + 1): their dwords are 80 = 16 (mod 32) banks apart and each covers 16 consecutive banks — no conflict.
//
// Arithmetic: the reference's types as compiled with -std=c++11 — float variables, every right-hand side with a double literal or
// h[] in it evaluated in double and rounded once at the assignment, pow(float, (int)2) the exact double product — in the
// reference's order, no contraction (the pragma below), IEEE division (hipcc's default), double exp.
#include "motion.h"

#pragma clang fp contract(off)

namespace dsdtm {

namespace {

constexpr int TILE_PX = 4 * MOTION_TILE_CELLS;             // 64
constexpr int LDS_SIDE = TILE_PX + 4;                      // 68 rows, 68 bytes of each used
constexpr int LDS_PITCH_DW = 20;                           // 80 bytes: see the bank note above
enum { MEAN = 0, VAR = 2, AGE = 4, MEAN_T = 6, VAR_T = 8, AGE_T = 10 };

__device__ __forceinline__ void order(int& a, int& b) {
    const int lo = min(a, b);
    b = max(a, b);
    a = lo;
}

// min of v[0..K) to v[0], max to v[K-1]
template <int K>
__device__ __forceinline__ void minmax(int (&v)[14]) {
#pragma unroll
    for (int i = 0; i < K / 2; ++i) order(v[i], v[K - 1 - i]);        // lows in front, highs behind; an odd middle joins both
#pragma unroll
    for (int i = 1; i < (K + 1) / 2; ++i) order(v[0], v[i]);
#pragma unroll
    for (int i = K / 2; i < K - 1; ++i) order(v[i], v[K - 1]);
}

// the 13th smallest of 25: hold 14, drop the smallest and the largest, take the next one in, ... until 3 are left
template <int K>
__device__ __forceinline__ int forget(int (&v)[14], const int (&e)[25]) {
    minmax<K>(v);
    if constexpr (K == 3) return v[1];
    else {
        v[0] = e[14 + (14 - K)];
        return forget<K - 1>(v, e);
    }
}

__device__ __forceinline__ int median25(const int (&e)[25]) {
    int v[14];
#pragma unroll
    for (int i = 0; i < 14; ++i) v[i] = e[i];
    return forget<14>(v, e);
}

__device__ __forceinline__ int clampi(int v, int hi) { return v < 0 ? 0 : v > hi ? hi : v; }

}  // namespace

__global__ __launch_bounds__(256) void motion_step_kernel(const MotionStepDev* __restrict__ recs) {
    const MotionStepDev& r = recs[blockIdx.z];
    const int mw = r.mw, mh = r.mh, width = r.width, height = r.height;
    if ((int)blockIdx.x * MOTION_TILE_CELLS >= mw || (int)blockIdx.y * MOTION_TILE_CELLS >= mh) return;      // a smaller model of the batch
    __shared__ uint32_t tile[LDS_SIDE * LDS_PITCH_DW];
    const int tid = threadIdx.x;
    const uint8_t* __restrict__ img = r.image;
    // ---- the tile with its halo: dword (row, q) holds pixels x0 + 4 q .. + 3 of image row y0 + row, coordinates clamped ----
    const int x0 = (int)blockIdx.x * TILE_PX - 2, y0 = (int)blockIdx.y * TILE_PX - 2;
    for (int s = tid; s < LDS_SIDE * (LDS_SIDE / 4); s += 256) {
        const int row = s / (LDS_SIDE / 4), q = s - row * (LDS_SIDE / 4);
        uint32_t v = 0;
        if (img) {
            const uint8_t* line = img + (size_t)clampi(y0 + row, height - 1) * (size_t)r.img_stride;
            const int x = x0 + 4 * q;
            if (x >= 0 && x + 3 < width && !(((size_t)(line + x)) & 3)) v = *(const uint32_t*)(line + x);
            else
                v = (uint32_t)line[clampi(x, width - 1)] | (uint32_t)line[clampi(x + 1, width - 1)] << 8 |
                    (uint32_t)line[clampi(x + 2, width - 1)] << 16 | (uint32_t)line[clampi(x + 3, width - 1)] << 24;
        }
        tile[row * LDS_PITCH_DW + q] = v;
    }
    __syncthreads();
    const int cx = tid & 15, cy = tid >> 4;
    const int i = (int)blockIdx.x * MOTION_TILE_CELLS + cx, j = (int)blockIdx.y * MOTION_TILE_CELLS + cy;
    if (i >= mw || j >= mh) return;
    // ---- 16 medians of 25 from the cell's 8 x 8 window ----
    int win[8][8];
#pragma unroll
    for (int rr = 0; rr < 8; ++rr) {
        const uint32_t a = tile[(4 * cy + rr) * LDS_PITCH_DW + cx], b = tile[(4 * cy + rr) * LDS_PITCH_DW + cx + 1];
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            win[rr][c] = (int)((a >> (8 * c)) & 0xffu);
            win[rr][4 + c] = (int)((b >> (8 * c)) & 0xffu);
        }
    }
    int px[16];
#pragma unroll
    for (int oy = 0; oy < 4; ++oy)
#pragma unroll
        for (int ox = 0; ox < 4; ++ox) {
            int e[25];
#pragma unroll
            for (int dy = 0; dy < 5; ++dy)
#pragma unroll
                for (int dx = 0; dx < 5; ++dx) e[5 * dy + dx] = win[oy + dy][ox + dx];
            px[4 * oy + ox] = median25(e);
        }
    const size_t nc = (size_t)mw * (size_t)mh;
    const size_t c = (size_t)i + (size_t)j * (size_t)mw;
    const float* __restrict__ src = r.src;
    float* __restrict__ dst = r.dst;
    auto old = [&](int arr, size_t at_) { return src ? src[(size_t)arr * nc + at_] : 0.0f; };
    // ---- motionCompensate (:183-367) ----
    const float X = (float)(4.0 * i + 4.0 / 2.0), Y = (float)(4.0 * j + 4.0 / 2.0);
    const float newW = (float)(r.H[6] * X + r.H[7] * Y + r.H[8]);
    const float newX = (float)((r.H[0] * X + r.H[1] * Y + r.H[2]) / newW);
    const float newY = (float)((r.H[3] * X + r.H[4] * Y + r.H[5]) / newW);
    const float newI = (float)(newX / 4.0), newJ = (float)(newY / 4.0);
    const float fI = floorf(newI), fJ = floorf(newJ);
    // an index of magnitude 2^30 or more (or NaN) is off the model: the reference's float -> int conversion is undefined there
    const bool okI = fabsf(fI) < 1073741824.0f, okJ = fabsf(fJ) < 1073741824.0f;
    const int iI = okI ? (int)fI : -2, iJ = okJ ? (int)fJ : -2;
    const float di = okI ? (float)(newI - ((float)iI + 0.5)) : 0.5f, dj = okJ ? (float)(newJ - ((float)iJ + 0.5)) : 0.5f;
    const int sI = di > 0 ? 1 : -1, sJ = dj > 0 ? 1 : -1;
    const float adi = fabsf(di), adj = fabsf(dj);
    // horizontal, vertical, diagonal, self — the reference's order
    const int nI[4] = {iI + sI, iI, iI + sI, iI}, nJ[4] = {iJ, iJ + sJ, iJ + sJ, iJ};
    const bool want[4] = {di != 0, dj != 0, di != 0 && dj != 0, true};
    const float wk[4] = {(float)(adi * (1.0 - adj)), (float)(adj * (1.0 - adi)), adi * adj, (float)((1.0 - adi) * (1.0 - adj))};
    bool in[4];
    size_t at[4];
    float wgt[4], sumW = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        in[k] = want[k] && okI && okJ && nI[k] >= 0 && nI[k] < mw && nJ[k] >= 0 && nJ[k] < mh;
        at[k] = in[k] ? (size_t)nI[k] + (size_t)nJ[k] * (size_t)mw : 0;
        wgt[k] = in[k] ? wk[k] : 0.0f;
        if (in[k]) sumW += wgt[k];
    }
    float t[6];            // this cell's m_Mean_Temp, m_Var_Temp, m_Age_Temp x 2 modes: what the previous step left (:277, :341)
#pragma unroll
    for (int k = 0; k < 6; ++k) t[k] = src ? src[(size_t)(MEAN_T + k) * nc + c] : 0.0f;          // (src == NULL: ProbModel::init, all zero)
    float* tM = t, *tV = t + 2, *tA = t + 4;
    if (sumW > 0) {
#pragma unroll
        for (int m = 0; m < 2; ++m) {
            float om[4], tm[4], ta[4], tv[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                om[k] = in[k] ? old(MEAN + m, at[k]) : 0.0f;
                tm[k] = in[k] ? wgt[k] * om[k] : 0.0f;
                ta[k] = in[k] ? wgt[k] * old(AGE + m, at[k]) : 0.0f;
            }
            tM[m] = (tm[0] + tm[1] + tm[2] + tm[3]) / sumW;
            tA[m] = (ta[0] + ta[1] + ta[2] + ta[3]) / sumW;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const float d = tM[m] - om[k];
                tv[k] = in[k] ? (float)(wgt[k] * (old(VAR + m, at[k]) + 1.0 * ((double)d * (double)d))) : 0.0f;
            }
            tV[m] = (tv[0] + tv[1] + tv[2] + tv[3]) / sumW;
        }
    }
    const bool border = iI < 1 || iI >= mw - 1 || iJ < 1 || iJ >= mh - 1;
#pragma unroll
    for (int m = 0; m < 2; ++m) {
        tV[m] = (float)(tV[m] < 30.0 * 30.0 ? 30.0 * 30.0 : tV[m]);                        // MAX(var, MIN_BG_VAR) (:355)
        if (border) { tV[m] = (float)(15.0 * 15.0); tA[m] = 0; }
        else {
            const double over = tV[m] - 50.0 * 50.0;
            const double a = tA[m] * exp(-(0.001) * (0.0 < over ? over : 0.0));
            tA[m] = (float)(a > 2.0 ? 2.0 : a);
        }
    }
    // ---- update, pass 1 (:392-456) ----
    float cur_mean = 0;
#pragma unroll
    for (int k = 0; k < 16; ++k) cur_mean += (float)px[k];
    cur_mean /= 16.0f;
    {
        int oldIdx = 0;
        float oldAge = 0;
        if (tA[0] >= oldAge) oldAge = tA[0];
        if (tA[1] >= oldAge) oldIdx = 1;               // >= : equal ages pick mode 1
        if (oldIdx != 0) {                             // not a swap: mode 0 receives mode 1, mode 1 starts over
            tM[0] = tM[1]; tM[1] = cur_mean;
            tV[0] = tV[1]; tV[1] = (float)(15.0 * 15.0);
            tA[0] = tA[1]; tA[1] = 0;
        }
    }
    int match;
    {
        const float d0 = cur_mean - tM[0], d1 = cur_mean - tM[1];
        if ((double)d0 * (double)d0 < 2.0 * tV[0]) match = 0;
        else if ((double)d1 * (double)d1 < 2.0 * tV[1]) match = 1;
        else { match = 1; tA[1] = 0; }
    }
    // ---- pass 2 (:463-511) ----
    float nM[2], nV[2], nA[2];
#pragma unroll
    for (int m = 0; m < 2; ++m) {
        const float age = tA[m], alpha = (float)(age / (age + 1.0));
        const float blend = (float)(alpha * tM[m] + (1.0 - alpha) * cur_mean);
        nM[m] = m != match ? tM[m] : age < 1 ? cur_mean : blend;
    }
    // ---- pass 3 (:512-580) ----
    const float mean_match = match == 0 ? nM[0] : nM[1];
    const bool old_enough = tA[0] > 1;
    const double fg_at = 2.0 * tV[0];                  // m_Var_Temp[0]: the variance from BEFORE this update (:546)
    float obs_var = 0;
    uint32_t mrow[4] = {0, 0, 0, 0};
#pragma unroll
    for (int k = 0; k < 16; ++k) {
        const float p = (float)px[k];
        const float fDiff = p - mean_match;
        const float pixelDist = (float)(0.0f + (double)fDiff * (double)fDiff);
        const float f0 = p - nM[0];
        const float dimg = (float)((double)f0 * (double)f0);
        if (old_enough && dimg > fg_at) mrow[k >> 2] |= 255u << (8 * (k & 3));
        obs_var = obs_var < pixelDist ? pixelDist : obs_var;
    }
#pragma unroll
    for (int m = 0; m < 2; ++m) {
        const float age = tA[m], alpha = (float)(age / (age + 1.0));
        float v = (float)(alpha * tV[m] + (1.0 - alpha) * obs_var);
        v = (float)(v < 30.0 * 30.0 ? 30.0 * 30.0 : v);
        const float first = (float)(obs_var < 15.0 * 15.0 ? 15.0 * 15.0 : obs_var);
        float a = (float)(age + 1.0);
        a = (float)(a > 2.0 ? 2.0 : a);
        nV[m] = m != match ? tV[m] : age == 0 ? first : v;
        nA[m] = m != match ? age : a;
    }
#pragma unroll
    for (int m = 0; m < 2; ++m) {
        dst[(size_t)(MEAN + m) * nc + c] = nM[m];
        dst[(size_t)(VAR + m) * nc + c] = nV[m];
        dst[(size_t)(AGE + m) * nc + c] = nA[m];
        dst[(size_t)(MEAN_T + m) * nc + c] = tM[m];
        dst[(size_t)(VAR_T + m) * nc + c] = tV[m];
        dst[(size_t)(AGE_T + m) * nc + c] = tA[m];
    }
    // ---- the mask: this cell's 4 x 4 pixels, a dword per row; the last cell column / row also clears what lies beyond 4 * model ----
    uint8_t* __restrict__ mask = r.mask;
    if (!mask) return;
    const size_t pitch = (size_t)r.mask_pitch;
#pragma unroll
    for (int jj = 0; jj < 4; ++jj) *(uint32_t*)(mask + (size_t)(4 * j + jj) * pitch + (size_t)(4 * i)) = mrow[jj];
    const int x_end = i == mw - 1 ? width : 4 * i + 4;
    for (int x = 4 * i + 4; x < x_end; ++x)
        for (int jj = 0; jj < 4; ++jj) mask[(size_t)(4 * j + jj) * pitch + (size_t)x] = 0;
    if (j == mh - 1)
        for (int y = 4 * mh; y < height; ++y)
            for (int x = 4 * i; x < x_end; ++x) mask[(size_t)y * pitch + (size_t)x] = 0;
}

// Frame::Motion_Removal's test (src/Frame.cpp:352) against the mask where it lies: cvRound rounds halves to even (rintf)
__global__ __launch_bounds__(256) void motion_features_kernel(const MotionStepDev* __restrict__ recs) {
    const MotionStepDev& r = recs[blockIdx.y];
    const int f = (int)blockIdx.x * 256 + (int)threadIdx.x;
    if (f >= r.n_feat) return;
    const float fx = rintf(r.feat[2 * (size_t)f]), fy = rintf(r.feat[2 * (size_t)f + 1]);
    uint8_t on = 0;
    if (fx >= 0.0f && fx < (float)r.width && fy >= 0.0f && fy < (float)r.height)        // (the host refused anything else)
        on = r.mask[(size_t)(int)fy * (size_t)r.mask_pitch + (size_t)(int)fx] == 255 ? 1 : 0;
    r.flags[f] = on;
}

hipError_t motion_step_launch(const MotionStepDev* recs, int n, int tiles_x, int tiles_y, hipStream_t stream) {
    hipLaunchKernelGGL(motion_step_kernel, dim3((unsigned)tiles_x, (unsigned)tiles_y, (unsigned)n), dim3(256), 0, stream, recs);
    return hipGetLastError();
}

hipError_t motion_features_launch(const MotionStepDev* recs, int n, int max_features, hipStream_t stream) {
    hipLaunchKernelGGL(motion_features_kernel, dim3((unsigned)((max_features + 255) / 256), (unsigned)n), dim3(256), 0, stream, recs);
    return hipGetLastError();
}

}  // namespace dsdtm
