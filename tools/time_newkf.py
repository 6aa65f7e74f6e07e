"""Times dsdtm_newkf_make(_batch) (libdsdtm_amd_newkf.so) on the MI355X and create_keyframe_host (dsdtm_amd/host/dsdtm_newkf_host.hpp,
one host thread) on the same seeded trackers: n = 1, 64, 1024 trackers of 300 cells (20 x 15, cell 32), 200 existing features, cap
400, 640x480; and the walk's worst case (G = 4096, every cell above the floor) with the cap out of reach and with the cap one feature
away, whose difference is what the sequential walk costs.

    python tools/time_newkf.py [--out FILE]

The times are host clocks around synchronous calls (each ends in a stream synchronise), the median of `--repeats` calls after warm-up.
The depth images lie in DEVICE memory for the device entry unless a row says pageable (then each call stages n x 614 KB through the
pinned block), and in ordinary host memory for the host function (the worst-case host row uses a depth image of another seed: the
lift's cost does not depend on the values). Both FULL paths of one tracker are run in C++ by tools/newkf_paths_timer.cpp on a resident
640x480 frame (cell 32, cap 400, min_dist 10, 200 existing features): the three round trips of the parent commit — Feature_detector::detect
of dsdtm_host.hpp (dsdtm_detect_cells_frame, then its sort / full-size mask / walk on one host thread) and dsdtm_frame_lift — and
dsdtm_detect_cells_frame + dsdtm_newkf_make, with the depth image in device, pinned and pageable memory. dsdtm_detect_cells_batch_device
is not timed. The generators and the case file format are those of tests/newkf_cases.py, which the tests of the entry use.
"""
import argparse
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HOST_TIMER = r"""
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include "dsdtm_amd/host/dsdtm_newkf_host.hpp"
template <class T> static std::vector<T> take(FILE* f, size_t n) { std::vector<T> v(n); if (n && fread(v.data(), sizeof(T), n, f) != n) exit(2); return v; }
int main(int argc, char** argv) {
    FILE* in = fopen(argv[1], "rb"); const int repeats = atoi(argv[2]);
    const int n = take<int32_t>(in, 1)[0];
    double total = 0; long sink = 0;
    for (int job = 0; job < n; ++job) {
        auto pi = take<int32_t>(in, 7); auto pf = take<float>(in, 5);
        dsdtm_newkf_params p{}; p.width = pi[0]; p.height = pi[1]; p.cell_size = pi[2]; p.grid_cols = pi[3]; p.grid_rows = pi[4]; p.max_fts = pi[5]; p.min_dist = pi[6]; p.score_floor = pf[0];
        dsdtm_camera cam{}; cam.fx = pf[1]; cam.fy = pf[2]; cam.cx = pf[3]; cam.cy = pf[4];
        const size_t G = (size_t)p.grid_cols * p.grid_rows, px = (size_t)p.width * p.height;
        auto s = take<float>(in, G); auto x = take<int32_t>(in, G), y = take<int32_t>(in, G), l = take<int32_t>(in, G);
        auto head = take<int32_t>(in, 2); const size_t ne = (size_t)head[0];
        auto epx = take<float>(in, 2 * ne); auto el = take<int32_t>(in, ne); auto eb = take<double>(in, 3 * ne);
        auto eh = take<uint8_t>(in, ne), ei = take<uint8_t>(in, ne); auto ep = take<int32_t>(in, ne);
        auto depth = take<uint16_t>(in, px); const float scale = take<float>(in, 1)[0]; const int has_dyn = take<int32_t>(in, 1)[0];
        auto dyn = take<uint8_t>(in, has_dyn ? px : 0); auto T = take<double>(in, 12);
        dsdtm_newkf_desc d{}; d.cell_score = s.data(); d.cell_x = x.data(); d.cell_y = y.data(); d.cell_level = l.data(); d.n_existing = head[0];
        d.first_point_index = head[1]; d.px_xy = epx.data(); d.level = el.data(); d.bearing = eb.data(); d.has_point = eh.data(); d.initial = ei.data();
        d.point_index = ep.data(); d.depth = depth.data(); d.depth_stride = p.width; d.depth_scale = scale; d.dyn_mask = has_dyn ? dyn.data() : nullptr;
        d.dyn_stride = p.width; d.T_c2w = T.data();
        std::vector<double> ts;
        for (int r = 0; r < repeats + 2; ++r) {
            const auto t0 = std::chrono::steady_clock::now();
            const DSDTM::NewKeyframeHost o = DSDTM::create_keyframe_host(cam, p, d);
            const auto t1 = std::chrono::steady_clock::now();
            sink += o.n_new_points;
            if (r >= 2) ts.push_back(std::chrono::duration<double, std::micro>(t1 - t0).count());
        }
        std::sort(ts.begin(), ts.end());
        total += ts[ts.size() / 2];
        printf("host job %d: %.1f us (median of %d)\n", job, ts[ts.size() / 2], repeats);
    }
    printf("host mean per tracker: %.1f us (sink %ld)\n", total / n, sink);
    return 0;
}
"""


def tracker(seed, prm, n_existing):
    from dsdtm_amd.keyframe_creation_restatement import NewKeyframeInput
    from tests import newkf_cases as cases
    rng = np.random.default_rng(seed)
    s, x, y, l = cases.random_cells(rng, prm, scores=tuple(np.linspace(5.0, 200.0, 120)))
    return NewKeyframeInput(s, x, y, l, cases.random_depth(rng, prm), 5000.0, cases.pose(rng), 1000, **cases.random_existing(rng, prm, n_existing, 1000))


def median_us(call, repeats, warmup=3):
    from dsdtm_amd import keyframe_creation as kc
    for _ in range(warmup):
        assert call.run_raw() == kc.OK, call.ctx.last_error()
    ts = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        st = call.run_raw()
        ts.append((time.perf_counter() - t0) * 1e6)
        assert st == kc.OK
    ts.sort()
    return ts[len(ts) // 2], ts[0], ts[-1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--repeats", type=int, default=50)
    a = ap.parse_args()
    import torch
    torch.cuda.init()
    from dsdtm_amd import keyframe_creation as kc
    from dsdtm_amd.keyframe_creation_restatement import NewKeyframeInput, NewKeyframeParams
    from tests import newkf_cases as cases
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    ctx = kc.NewKeyframeContext(0)
    prm = NewKeyframeParams(640, 480, 32, 20, 15, 400, 10, 20.0)
    base = [tracker(s, prm, 200) for s in range(8)]
    dev_depth = []
    for b in base:
        t = torch.from_numpy(np.ascontiguousarray(b.depth).view(np.int16)).cuda()
        dev_depth.append(kc.DeviceArray(t.data_ptr(), 640, t))
    torch.cuda.synchronize()
    say(f"device: {torch.cuda.get_device_name(0)}; 300 cells, 200 existing, cap 400, 640x480; median [min, max] of {a.repeats} calls, us")
    for n in (1, 64, 1024):
        dev = [NewKeyframeInput(**{**base[t % 8].__dict__, "depth": dev_depth[t % 8]}) for t in range(n)]
        m, lo, hi = median_us(kc.MakeCall(ctx, cases.CAM, prm, dev), a.repeats)
        say(f"dsdtm_newkf_make_batch n={n:5d} depth in device memory  : {m:10.1f} [{lo:.1f}, {hi:.1f}]  = {m / n:.2f} per tracker")
        if n <= 64:
            m, lo, hi = median_us(kc.MakeCall(ctx, cases.CAM, prm, [base[t % 8] for t in range(n)]), a.repeats)
            say(f"dsdtm_newkf_make_batch n={n:5d} depth in pageable memory: {m:10.1f} [{lo:.1f}, {hi:.1f}]  = {m / n:.2f} per tracker")
    # the walk's worst case: the same 4096 candidates with the cap out of reach and with the cap one feature away
    big = NewKeyframeParams(1024, 1024, 16, 64, 64, 100000, 8, 20.0)
    rng = np.random.default_rng(4096)
    s, x, y, l = cases.random_cells(rng, big, scores=tuple(np.linspace(21.0, 500.0, 700)))
    worst = NewKeyframeInput(s, x, y, l, cases.random_depth(rng, big), 5000.0, cases.pose(rng), 7, **cases.random_existing(rng, big, 50, 7))
    t = torch.from_numpy(np.ascontiguousarray(worst.depth).view(np.int16)).cuda()
    worst.depth = kc.DeviceArray(t.data_ptr(), 1024, t)
    full = kc.MakeCall(ctx, cases.CAM, big, [worst])
    m_full, lo, hi = median_us(full, a.repeats)
    n_acc = full.results[0].n_new
    say(f"worst case G=4096, {n_acc} accepted, walk to the end       : {m_full:10.1f} [{lo:.1f}, {hi:.1f}]")
    short = NewKeyframeParams(1024, 1024, 16, 64, 64, 51, 8, 20.0)
    m_short, lo, hi = median_us(kc.MakeCall(ctx, cases.CAM, short, [worst]), a.repeats)
    say(f"worst case G=4096, cap after one acceptance (sort + K3 only): {m_short:10.1f} [{lo:.1f}, {hi:.1f}]")
    say(f"  the walk and the {n_acc} extra slots: {m_full - m_short:.1f} us of {m_full:.1f}")
    ctx.close()
    # the host function on the same eight trackers and on the worst case
    with tempfile.TemporaryDirectory() as tmp:
        src, exe = os.path.join(tmp, "timer.cpp"), os.path.join(tmp, "timer")
        open(src, "w").write(HOST_TIMER)
        subprocess.run(["g++", "-O2", "-std=c++14", "-ffp-contract=off", "-I", ROOT, "-o", exe, src], check=True)
        worst.depth = np.ascontiguousarray(cases.random_depth(np.random.default_rng(1), big))
        for name, cs in (("300 cells", [dict(prm=prm, inp=b) for b in base]), ("worst case G=4096", [dict(prm=big, inp=worst)])):
            open(os.path.join(tmp, "cases.bin"), "wb").write(cases.pack(cs))
            out = subprocess.run([exe, os.path.join(tmp, "cases.bin"), str(a.repeats)], capture_output=True, text=True, check=True).stdout
            say(f"create_keyframe_host, one host thread, {name}: {out.strip().splitlines()[-1]}")
    # both FULL paths for one tracker, in C++ (tools/newkf_paths_timer.cpp): the parent commit's three round trips — Feature_detector::detect
    # of dsdtm_host.hpp (detect cells, then its walk with a full-size mask on one host thread), then dsdtm_frame_lift — and the new path
    from dsdtm_amd import synth
    exe = os.path.join(ROOT, "tools", "newkf_paths_timer")
    if not os.path.exists(exe):
        csrc = os.path.join(ROOT, "dsdtm_amd", "csrc")
        subprocess.run([os.environ.get("HIPCC", "hipcc"), "-std=c++17", "-O2", "-ffp-contract=off", "-I", ROOT, exe + ".cpp", "-L", csrc, "-ldsdtm_amd",
                        "-ldsdtm_amd_newkf", "-ldsdtm_amd_mapping", "-Wl,-rpath," + csrc, "-o", exe], check=True)
    img = np.clip(np.rint(synth.make_texture(480, 640, 99)), 0, 255).astype(np.uint8)
    ex = np.asarray(base[0].px_xy, np.float32).clip(0, [639, 479]).astype(np.float32)
    with tempfile.TemporaryDirectory() as tmp:
        scene = os.path.join(tmp, "scene.bin")
        with open(scene, "wb") as f:
            f.write(np.asarray([640, 480, len(ex)], np.int32).tobytes() + img.tobytes() + np.ascontiguousarray(base[0].depth, np.uint16).tobytes()
                    + ex.tobytes() + np.ascontiguousarray(base[0].initial, np.uint8).tobytes() + np.ascontiguousarray(base[0].T_c2w, np.float64).tobytes())
        r = subprocess.run([exe, scene, str(a.repeats)], capture_output=True, text=True)
        for line in r.stdout.strip().splitlines():
            say(line)
        assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
