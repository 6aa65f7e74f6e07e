"""dsdtm_need_keyframes against need_keyframe_host: wall time per call of the device entry for n trackers, and the same
trackers through the plain host function (dsdtm_host.hpp) on one thread, timed by a small C++ loop that is built below.

    python tools/need_keyframe_bench.py [--reps 7] [--calls 200] [--out profiles/r13_need_keyframe.txt]
    rocprofv3 --kernel-trace --stats ... -- python tools/need_keyframe_bench.py --only-device 1024 --calls 200     # kernel time

Per batch size n in (1, 8, 64, 256, 1024): trackers of 200 current points, 300 keyframe points, 10 local keyframes (seeded;
tests/need_keyframe_cases.random_case). A repetition times `--calls` calls of either path back to back, alternating the two
paths; the report is the median and the spread (min .. max) of the per-repetition means, after a warm-up. Both paths are checked
against each other on the timed inputs before anything is timed."""
import argparse
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HOST_TIMER = r'''
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "dsdtm_host.hpp"
// usage: timer <cases.bin> <calls> <reps>: the cases of tests/need_keyframe_cases.write_cases; prints one line per repetition:
// microseconds per pass over all trackers (one thread), and a checksum so that nothing is optimised away
template <typename T> static void rd(FILE* f, T* p, size_t n) { if (n && std::fread(p, sizeof(T), n, f) != n) std::exit(2); }
struct Case { std::vector<double> Tc, Tk, pc, pk, cen; std::vector<uint8_t> bc, bk; };
int main(int argc, char** argv) {
    FILE* f = std::fopen(argv[1], "rb");
    const int calls = std::atoi(argv[2]), reps = std::atoi(argv[3]);
    int32_t n; rd(f, &n, 1);
    float camf[4]; rd(f, camf, 4);
    const dsdtm_camera cam{camf[0], camf[1], camf[2], camf[3], camf[0], 640, 480};
    std::vector<Case> cs((size_t)n); std::vector<dsdtm_keyframe_desc> ds((size_t)n); std::vector<dsdtm_keyframe_params> ps((size_t)n);
    for (int t = 0; t < n; ++t) {
        Case& c = cs[(size_t)t]; dsdtm_keyframe_desc& d = ds[(size_t)t]; dsdtm_keyframe_params& p = ps[(size_t)t];
        int32_t ip[3], counts[4], has_bad[2]; double dp[3];
        rd(f, ip, 3); rd(f, dp, 3);
        p.min_valid = ip[0]; p.max_valid = ip[1]; p.px_samples = ip[2]; p.reserved = 0; p.min_px_median = dp[0]; p.min_rot = dp[1]; p.min_trans = dp[2];
        c.Tc.resize(12); c.Tk.resize(12); rd(f, c.Tc.data(), 12); rd(f, c.Tk.data(), 12); rd(f, counts, 4); rd(f, has_bad, 2);
        c.pc.resize(3 * (size_t)counts[1]); c.bc.resize((size_t)counts[1]); c.pk.resize(3 * (size_t)counts[2]); c.bk.resize((size_t)counts[2]);
        c.cen.resize(3 * (size_t)counts[3]);
        rd(f, c.pc.data(), c.pc.size()); rd(f, c.bc.data(), c.bc.size()); rd(f, c.pk.data(), c.pk.size()); rd(f, c.bk.data(), c.bk.size());
        rd(f, c.cen.data(), c.cen.size());
        d.T_cur_w = c.Tc.data(); d.T_kf_w = c.Tk.data(); d.n_valid = counts[0]; d.n_cur_points = counts[1]; d.cur_p_world = c.pc.data();
        d.cur_bad = has_bad[0] ? c.bc.data() : nullptr; d.n_kf_points = counts[2]; d.kf_p_world = c.pk.data();
        d.kf_bad = has_bad[1] ? c.bk.data() : nullptr; d.n_local_kf = counts[3]; d.local_kf_centre = c.cen.data();
    }
    double sum = 0;
    for (int r = 0; r < reps + 1; ++r) {             // (the first repetition is the warm-up)
        const auto t0 = std::chrono::steady_clock::now();
        for (int k = 0; k < calls; ++k)
            for (int t = 0; t < n; ++t) { dsdtm_keyframe_verdict v; DSDTM::need_keyframe_host(cam, ps[(size_t)t], ds[(size_t)t], &v); sum += v.median_depth + v.need; }
        const double us = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count() / calls;
        if (r) std::printf("%.3f\n", us);
    }
    std::fprintf(stderr, "checksum %.17g\n", sum);
    return 0;
}
'''


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--sizes", default="1,8,64,256,1024")
    ap.add_argument("--only-device", type=int, default=0, metavar="N", help="N trackers, --calls device calls and nothing else (for rocprofv3)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from dsdtm_amd import capi
    from tests import need_keyframe_cases as cases
    ctx = capi.KeyframeContext(0)

    def batch(n):
        return [cases.random_case(9000 + t % 64, 200, 300, 10, bad="some", fire=(9 if t % 3 == 0 else None)) for t in range(n)]

    if a.only_device:
        call = capi.KeyframeCall(ctx, cases.CAM, None, [cases.desc_of(c) for c in batch(a.only_device)])
        for _ in range(a.calls):
            ctx.check(call.run_raw())
        return
    tmp = tempfile.mkdtemp()
    src, exe = os.path.join(tmp, "timer.cpp"), os.path.join(tmp, "timer")
    with open(src, "w") as f:
        f.write(HOST_TIMER)
    lib = capi.keyframe_lib_path()
    subprocess.run(["g++", "-O2", "-std=c++14", "-ffp-contract=off", "-I", os.path.join(ROOT, "dsdtm_amd", "host"), "-o", exe, src, lib,
                    "-Wl,-rpath," + os.path.dirname(lib), "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib", "-lamdhip64"], check=True)
    lines = [f"dsdtm_need_keyframes vs need_keyframe_host: 200 current points, 300 keyframe points, 10 local keyframes per tracker; "
             f"{a.reps} repetitions of {a.calls} calls, alternating; microseconds per call (all n trackers), median [min .. max]",
             lib_line(capi)]
    rows = []
    for n in [int(v) for v in a.sizes.split(",")]:
        cs = batch(n)
        call = capi.KeyframeCall(ctx, cases.CAM, None, [cases.desc_of(c) for c in cs])
        got = call.run()
        for g, c in zip(got, cs):
            cases.assert_same_verdict(g, cases.run_reference(c), ("bench", n))
        path = os.path.join(tmp, f"cases_{n}.bin")
        cases.write_cases(path, cs)
        for _ in range(50):
            ctx.check(call.run_raw())
        dev, host = [], []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            for _ in range(a.calls):
                st = call.run_raw()
            dev.append((time.perf_counter() - t0) / a.calls * 1e6)
            ctx.check(st)
            out = subprocess.run([exe, path, str(max(1, a.calls // max(1, n // 8))), "1"], capture_output=True, text=True, check=True).stdout
            host.append(float(out.split()[0]))
        rows.append((n, np.median(dev), min(dev), max(dev), np.median(host), min(host), max(host)))
        lines.append(f"n = {n:5d}   device {np.median(dev):9.1f} [{min(dev):9.1f} .. {max(dev):9.1f}]   host, one thread {np.median(host):9.1f} "
                     f"[{min(host):9.1f} .. {max(host):9.1f}]   device / host {np.median(dev) / np.median(host):6.2f}")
    cross = next((n for n, d, _, _, h, _, _ in rows if d < h), None)
    lines.append(f"crossover: the device entry is faster from n = {cross} (of the sizes measured)" if cross else
                 "crossover: none — the host function is faster at every measured n")
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


def lib_line(capi):
    import hashlib
    with open(capi.keyframe_lib_path(), "rb") as f:
        return "library " + capi.KEYFRAME_LIB_NAME + " sha256 " + hashlib.sha256(f.read()).hexdigest()[:16]


if __name__ == "__main__":
    main()
