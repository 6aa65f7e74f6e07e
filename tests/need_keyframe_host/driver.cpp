// need_keyframe_host (dsdtm_amd/host/dsdtm_host.hpp) and dsdtm_need_keyframes on the same trackers: reads the cases
// tests/test_need_keyframe_gpu.py writes and prints both verdicts with 17 digits. Test infrastructure only.
//   usage: driver <cases.bin> [host]      host: need_keyframe_host only (no device, no context)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../dsdtm_amd/host/dsdtm_host.hpp"

template <typename T>
static void rd(FILE* f, T* p, size_t n) {
    if (n && std::fread(p, sizeof(T), n, f) != n) { std::fprintf(stderr, "short read\n"); std::exit(2); }
}

struct Case {
    std::vector<double> Tc, Tk, pc, pk, cen;
    std::vector<uint8_t> bc, bk;
};

static void print(const char* who, int t, const dsdtm_keyframe_verdict& v) {
    std::printf("%s %d %d %d %d %d %d %d %d %.17g %.17g %.17g %.17g %.17g\n", who, t, v.need, v.reason, v.rule_mask, v.undefined, v.n_px, v.n_depth,
                v.svo_kf, v.median_px, v.rot, v.trans, v.min_depth, v.median_depth);
}

int main(int argc, char** argv) {
    if (argc < 2) { std::fprintf(stderr, "usage: %s cases.bin [host]\n", argv[0]); return 2; }
    FILE* f = std::fopen(argv[1], "rb");
    if (!f) { std::perror("open"); return 2; }
    int32_t n;
    rd(f, &n, 1);
    float camf[4];
    rd(f, camf, 4);
    const dsdtm_camera cam{camf[0], camf[1], camf[2], camf[3], camf[0], 640, 480};
    std::vector<Case> cs((size_t)n);
    std::vector<dsdtm_keyframe_desc> ds((size_t)n);
    std::vector<dsdtm_keyframe_params> ps((size_t)n);
    for (int t = 0; t < n; ++t) {
        Case& c = cs[(size_t)t];
        dsdtm_keyframe_desc& d = ds[(size_t)t];
        int32_t ip[3], counts[4], has_bad[2];
        double dp[3];
        rd(f, ip, 3); rd(f, dp, 3);
        dsdtm_keyframe_params& p = ps[(size_t)t];
        p.min_valid = ip[0]; p.max_valid = ip[1]; p.px_samples = ip[2]; p.reserved = 0; p.min_px_median = dp[0]; p.min_rot = dp[1]; p.min_trans = dp[2];
        c.Tc.resize(12); c.Tk.resize(12);
        rd(f, c.Tc.data(), 12); rd(f, c.Tk.data(), 12);
        rd(f, counts, 4); rd(f, has_bad, 2);
        c.pc.resize(3 * (size_t)counts[1]); c.bc.resize((size_t)counts[1]); c.pk.resize(3 * (size_t)counts[2]); c.bk.resize((size_t)counts[2]);
        c.cen.resize(3 * (size_t)counts[3]);
        rd(f, c.pc.data(), c.pc.size()); rd(f, c.bc.data(), c.bc.size());
        rd(f, c.pk.data(), c.pk.size()); rd(f, c.bk.data(), c.bk.size());
        rd(f, c.cen.data(), c.cen.size());
        d.T_cur_w = c.Tc.data(); d.T_kf_w = c.Tk.data(); d.n_valid = counts[0];
        d.n_cur_points = counts[1]; d.cur_p_world = c.pc.data(); d.cur_bad = has_bad[0] ? c.bc.data() : nullptr;
        d.n_kf_points = counts[2]; d.kf_p_world = c.pk.data(); d.kf_bad = has_bad[1] ? c.bk.data() : nullptr;
        d.n_local_kf = counts[3]; d.local_kf_centre = c.cen.data();
    }
    std::fclose(f);
    for (int t = 0; t < n; ++t) {
        dsdtm_keyframe_verdict v;
        DSDTM::need_keyframe_host(cam, ps[(size_t)t], ds[(size_t)t], &v);
        print("host", t, v);
    }
    if (argc > 2 && std::string(argv[2]) == "host") return 0;
    dsdtm_keyframe_ctx* kctx = nullptr;
    if (dsdtm_keyframe_create(0, &kctx) != DSDTM_OK) { std::fprintf(stderr, "dsdtm_keyframe_create: %s\n", dsdtm_keyframe_last_error(nullptr)); return 1; }
    for (int t = 0; t < n; ++t) {          // (the parameters differ per case: one call each)
        dsdtm_keyframe_verdict v;
        if (dsdtm_need_keyframe(kctx, &cam, &ps[(size_t)t], &ds[(size_t)t], &v) != DSDTM_OK) {
            std::fprintf(stderr, "dsdtm_need_keyframe: %s\n", dsdtm_keyframe_last_error(kctx));
            return 1;
        }
        print("device", t, v);
    }
    dsdtm_keyframe_destroy(kctx);
    return 0;
}
