// rarsac_api.cpp — the C ABI of include/dsdtm_amd_rarsac.h (libdsdtm_amd_rarsac.so): checks, packing, launch (the context: addon_host.h).
//
// A call checks every desc — R1 among the checks: the bin of every correspondence (the host header's bin_of: one definition for the
// library and the host path) — and, on the way, sorts each problem's correspondences by bin (a stable counting sort) and derives
// its table (R2's probabilities, R3's prefix sums). Records, tables and sorted correspondences go into one pinned block and move with
// a single hipMemcpyAsync; rarsac.hip's kernel (one workgroup per problem) runs on the context's stream; results and statuses come back
// with one copy; the caller's arrays are written only after the wait succeeded (the status back in the caller's order). There is no CPU
// compute path here: no hypothesis is drawn, solved or scored on the host.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <vector>

#include "rarsac.h"
#include "addon_host.h"
#define DSDTM_RARSAC_HOST_ONLY 1
#include "../host/dsdtm_rarsac_host.hpp"

using namespace dsdtm;

struct dsdtm_rarsac_ctx : dsdtm::AddonCtx {};

extern "C" const char* dsdtm_rarsac_last_error(const dsdtm_rarsac_ctx* ctx) { return addon_last_error(ctx); }
extern "C" int dsdtm_rarsac_create(int device, dsdtm_rarsac_ctx** out) { return addon_create("dsdtm_amd_rarsac", device, out); }
extern "C" void dsdtm_rarsac_destroy(dsdtm_rarsac_ctx* ctx) { addon_destroy(ctx); }

// what is wrong with one desc, or nullptr; `detail` receives the index where one is named
static const char* check_desc(const dsdtm_rarsac_desc& d, bool check, int* detail) {
    *detail = -1;
    if (d.m < DSDTM_RARSAC_MIN_POINTS || d.m > DSDTM_RARSAC_MAX_POINTS) return "m out of range";
    if (!d.cur) return "cur is NULL";
    if (!d.prev) return "prev is NULL";
    if (d.width < DSDTM_RARSAC_MIN_SIDE || d.width > DSDTM_RARSAC_MAX_SIDE) return "width out of range";
    if (d.height < DSDTM_RARSAC_MIN_SIDE || d.height > DSDTM_RARSAC_MAX_SIDE) return "height out of range";
    if (!std::isfinite(d.sigma) || d.sigma < 0.0f) return "sigma is not finite or negative";
    if (check) {
        if (!d.F) return "F is NULL";
        for (int j = 0; j < 9; ++j) if (!std::isfinite(d.F[j])) { *detail = j; return "F is not finite at entry"; }
    } else {
        if (d.max_iterations < 0 || d.max_iterations > DSDTM_RARSAC_MAX_ITERATIONS) return "max_iterations out of range";
        if (!std::isfinite(d.terminate_threshold) || d.terminate_threshold < 0.0) return "terminate_threshold is not finite or negative";
        double sum = 0.0;
        for (int j = 0; j < RARSAC_GRID; ++j) {
            if (!(d.grid_probability_in[j] >= 0.0 && d.grid_probability_in[j] <= 1.0)) { *detail = j; return "grid_probability_in outside 0..1 at bin"; }
            sum = sum + d.grid_probability_in[j];
        }
        if (!(sum > 0.0)) return "grid_probability_in sums to 0";
    }
    return nullptr;
}

static int submit(dsdtm_rarsac_ctx* ctx, const char* who, bool check, int n, const dsdtm_rarsac_desc* descs, dsdtm_rarsac_result* results) {
    if (!ctx) return DSDTM_ERR_INVALID;
    if (n < 0 || n > DSDTM_RARSAC_MAX_PROBLEMS) { set_err(ctx, "%s: n = %d outside 0..%d", who, n, DSDTM_RARSAC_MAX_PROBLEMS); return DSDTM_ERR_INVALID; }
    if (n == 0) return DSDTM_OK;
    if (!descs) { set_err(ctx, "%s: descs is NULL", who); return DSDTM_ERR_INVALID; }
    if (!results) { set_err(ctx, "%s: results is NULL", who); return DSDTM_ERR_INVALID; }
    {   // (the call allocates and waits: neither can be part of a capture)
        hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
        if (hipStreamIsCapturing(ctx->stream, &cs) != hipSuccess) { (void)hipGetLastError(); cs = hipStreamCaptureStatusNone; }
        if (cs != hipStreamCaptureStatusNone) { set_err(ctx, "%s: not inside a stream capture", who); return DSDTM_ERR_INVALID; }
    }
    // every desc is checked before anything is enqueued, R1 included: bins[] holds the bin of every correspondence of every problem
    const size_t N = (size_t)n;
    std::vector<size_t> first(N + 1, 0);
    for (int t = 0; t < n; ++t) {
        int detail = -1;
        if (const char* bad = check_desc(descs[t], check, &detail)) {
            if (detail >= 0) set_err(ctx, "%s: problem %d: %s %d", who, t, bad, detail);
            else set_err(ctx, "%s: problem %d: %s", who, t, bad);
            return DSDTM_ERR_INVALID;
        }
        first[(size_t)t + 1] = first[(size_t)t] + (size_t)descs[t].m;
    }
    std::vector<uint8_t> bins(first[N]);
    for (int t = 0; t < n; ++t) {
        const dsdtm_rarsac_desc& d = descs[t];
        const int gr = d.height / 10, gc = d.width / 10;
        for (int i = 0; i < d.m; ++i) {
            const float* c = d.cur + 2 * (size_t)i;
            const float* p = d.prev + 2 * (size_t)i;
            if (!std::isfinite(c[0]) || !std::isfinite(c[1])) { set_err(ctx, "%s: problem %d: cur is not finite at index %d", who, t, i); return DSDTM_ERR_INVALID; }
            if (!std::isfinite(p[0]) || !std::isfinite(p[1])) { set_err(ctx, "%s: problem %d: prev is not finite at index %d", who, t, i); return DSDTM_ERR_INVALID; }
            const int b = rarsac_detail::bin_of(c[0], c[1], gr, gc);
            if (b < 0) { set_err(ctx, "%s: problem %d: cur lies outside the 10x10 grid (R1) at index %d", who, t, i); return DSDTM_ERR_INVALID; }
            bins[first[(size_t)t] + (size_t)i] = (uint8_t)b;
        }
    }
    // the block: records | per problem: table, sorted correspondences (m x 4 floats) || results | per problem: status (m bytes up to 16)
    std::vector<size_t> table_at(N, 0), pt_at(N, 0), status_at(N, 0);
    size_t o = align_up(N * sizeof(RarsacDev), 256);
    for (int t = 0; t < n; ++t) {
        table_at[(size_t)t] = o; o += align_up(sizeof(RarsacTable), 16);
        pt_at[(size_t)t] = o; o += (size_t)descs[t].m * 16;
    }
    const size_t in_bytes = o;
    o = align_up(o, 256);
    const size_t out_begin = o;
    o += align_up(N * sizeof(dsdtm_rarsac_result), 16);
    for (int t = 0; t < n; ++t) { status_at[(size_t)t] = o; o += align_up((size_t)descs[t].m, 16); }
    const size_t out_end = o;
    if (int rc = ensure_stage(ctx, out_end, out_end)) return rc;
    uint8_t* h = (uint8_t*)ctx->h_pinned;
    uint8_t* g = (uint8_t*)ctx->d_stage;
    std::vector<uint16_t> order(first[N]);                  // sorted position -> correspondence, per problem
    for (int t = 0; t < n; ++t) {
        const dsdtm_rarsac_desc& d = descs[t];
        const uint8_t* bin = bins.data() + first[(size_t)t];
        uint16_t* ord = order.data() + first[(size_t)t];
        RarsacTable tab;
        memset(&tab, 0, sizeof tab);
        int count[RARSAC_GRID] = {0}, fill[RARSAC_GRID];
        for (int i = 0; i < d.m; ++i) count[bin[i]]++;
        tab.start[0] = 0;
        for (int j = 0; j < RARSAC_GRID; ++j) { tab.start[j + 1] = tab.start[j] + count[j]; fill[j] = tab.start[j]; }
        float* pt = (float*)(h + pt_at[(size_t)t]);
        for (int i = 0; i < d.m; ++i) {
            const int at = fill[bin[i]]++;
            ord[at] = (uint16_t)i;
            pt[4 * at] = d.cur[2 * i]; pt[4 * at + 1] = d.cur[2 * i + 1]; pt[4 * at + 2] = d.prev[2 * i]; pt[4 * at + 3] = d.prev[2 * i + 1];
        }
        double sum = 0.0;
        for (int j = 0; j < RARSAC_GRID; ++j) sum = sum + (check ? 0.5 : d.grid_probability_in[j]);
        int nb = 0, total = 0;
        for (int j = 0; j < RARSAC_GRID; ++j) {
            const double prior = check ? 0.5 : d.grid_probability_in[j];
            tab.prior[j] = prior;
            tab.binp[j] = prior / sum;
            if (count[j] > 0) {
                int w = (int)(prior * 1024.0);
                if (w < 1) w = 1;
                total += w;
                tab.nbin[nb] = j; tab.cum[nb] = total;
                ++nb;
            }
        }
        memcpy(h + table_at[(size_t)t], &tab, sizeof tab);
        RarsacDev r;
        memset(&r, 0, sizeof r);
        r.pt = (const float*)(g + pt_at[(size_t)t]);
        r.table = (const RarsacTable*)(g + table_at[(size_t)t]);
        r.status = g + status_at[(size_t)t];
        r.out = (dsdtm_rarsac_result*)(g + out_begin) + t;
        r.terminate = d.terminate_threshold > 0.0 ? d.terminate_threshold : DSDTM_RARSAC_DEFAULT_TERMINATE;
        const float sigma = d.sigma > 0.0f ? d.sigma : (float)DSDTM_RARSAC_DEFAULT_SIGMA;
        const float s2 = sigma * sigma;
        r.inv_sigma2 = (float)(1.0 / (double)s2);
        if (check) memcpy(r.F, d.F, sizeof r.F);
        r.seed = d.seed ? d.seed : DSDTM_RARSAC_DEFAULT_SEED;
        r.m = d.m; r.nb = nb; r.total = total; r.gr = d.height / 10; r.gc = d.width / 10;
        r.max_iterations = d.max_iterations > 0 ? d.max_iterations : DSDTM_RARSAC_DEFAULT_ITERATIONS;
        r.check = check ? 1 : 0;
        memcpy(h + (size_t)t * sizeof r, &r, sizeof r);
    }
    // (a failure behind the first enqueue waits for the stream: the pinned block is the next call's)
    auto fail = [&](int rc) { (void)hipStreamSynchronize(ctx->stream); return rc; };
    HIP_TRY(ctx, hipMemcpyAsync(g, h, in_bytes, hipMemcpyHostToDevice, ctx->stream));
    API_TRY(rarsac_launch((const RarsacDev*)g, n, ctx->stream));
    API_TRY(hipMemcpyAsync(h + out_begin, g + out_begin, out_end - out_begin, hipMemcpyDeviceToHost, ctx->stream));
    API_TRY(hipStreamSynchronize(ctx->stream));
    for (int t = 0; t < n; ++t) {
        dsdtm_rarsac_result got;
        memcpy(&got, h + out_begin + (size_t)t * sizeof got, sizeof got);
        if (got.found != 1) { results[t].found = 0; continue; }          // nothing else is written
        results[t] = got;
        if (descs[t].status) {
            const uint8_t* sorted = h + status_at[(size_t)t];
            const uint16_t* ord = order.data() + first[(size_t)t];
            for (int i = 0; i < descs[t].m; ++i) descs[t].status[ord[i]] = sorted[i];
        }
    }
    return DSDTM_OK;
}

extern "C" int dsdtm_rarsac_reject_batch(dsdtm_rarsac_ctx* ctx, int n, const dsdtm_rarsac_desc* descs, dsdtm_rarsac_result* results) {
    return submit(ctx, "rarsac_reject_batch", false, n, descs, results);
}

extern "C" int dsdtm_rarsac_check(dsdtm_rarsac_ctx* ctx, int n, const dsdtm_rarsac_desc* descs_with_F, dsdtm_rarsac_result* results) {
    return submit(ctx, "rarsac_check", true, n, descs_with_F, results);
}

extern "C" int dsdtm_rarsac_reject(dsdtm_rarsac_ctx* ctx, int m, const float* cur, const float* prev, int width, int height, const double* grid_probability_in,
                                   uint8_t* status, dsdtm_rarsac_result* result) {
    dsdtm_rarsac_desc d;
    memset(&d, 0, sizeof d);
    d.cur = cur; d.prev = prev; d.status = status; d.m = m; d.width = width; d.height = height;
    for (int j = 0; j < RARSAC_GRID; ++j) d.grid_probability_in[j] = grid_probability_in ? grid_probability_in[j] : 0.5;
    return submit(ctx, "rarsac_reject_batch", false, 1, &d, result);
}
