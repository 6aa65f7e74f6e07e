"""Wall time of dsdtm_framediff_steps at 640x480 for n = 1, 64 and 1024 pairs — images device-resident and pageable, the mask read back
and flags only — alternated in ONE process with frame_diff_host on one host thread (tools/framediff_host_timer.cpp: this repository's
own C++, NOT OpenCV). Each figure is the median of `--rounds` rounds of `--reps` calls behind a warm-up; device and host rounds take turns.

    python tools/time_framediff.py [--rounds 7] [--lib PATH]      # PATH: a library built with another -DFRAMEDIFF_ROWS, for the choice of R
    rocprofv3 --kernel-trace --stats -- python tools/time_framediff.py --trace      # n = 1024, device-resident, flags only: the kernel's time
"""
import argparse
import ctypes as C
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
W, H = 640, 480


def host_timer():
    so = os.path.join(ROOT, "tools", "libframediff_host_timer.so")
    src = os.path.join(ROOT, "tools", "framediff_host_timer.cpp")
    if not os.path.exists(so) or os.path.getmtime(so) < os.path.getmtime(src):
        subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", "-I", os.path.join(ROOT, "include"), "-o", so, src], check=True)
    lib = C.CDLL(so)
    lib.framediff_host_time_us.restype = C.c_double
    lib.framediff_host_time_us.argtypes = [C.c_void_p] * 2 + [C.c_int] * 2 + [C.c_void_p] + [C.c_int] * 3 + [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
    return lib


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--lib", default=None, help="another build of libdsdtm_amd_framediff.so (e.g. -DFRAMEDIFF_ROWS=16)")
    ap.add_argument("--trace", action="store_true", help="n = 1024 device-resident, flags only, 20 calls: for rocprofv3 --kernel-trace --stats")
    a = ap.parse_args()
    import torch
    from dsdtm_amd import _addon, framediff
    from tests import framediff_cases as cases
    if a.lib:
        _addon.lib_path = lambda name, _p=os.path.abspath(a.lib): _p
        framediff.lib_path = lambda: os.path.abspath(a.lib)
    ctx = framediff.FrameDiffContext(0)
    c = cases.by_name("640x480")
    want = cases.restated("640x480")
    feats = c["features"]
    a_dev, b_dev = torch.from_numpy(c["a"]).cuda(), torch.from_numpy(c["b"]).cuda()
    torch.cuda.synchronize()

    def prepared(n, resident, want_mask):
        img = (a_dev, b_dev) if resident else (c["a"], c["b"])
        return ctx.prepare([dict(a=img[0], b=img[1], H=c["H"], flags=c["flags"], threshold=c["threshold"], maxval=c["maxval"], features=feats,
                                 mask=True if want_mask else None) for _ in range(n)])

    def device_us(p, reps):
        t0 = time.perf_counter()
        for _ in range(reps):
            assert p.run_raw() == 0, ctx.last_error()
        return (time.perf_counter() - t0) * 1e6 / reps

    if a.trace:
        p = prepared(1024, True, False)
        for _ in range(20):
            assert p.run_raw() == 0, ctx.last_error()
        r = p.results()
        assert all(x["n_foreground"] == want["n_foreground"] and x["n_flagged"] == want["n_flagged"] for x in r)
        print("trace: 20 calls of n = 1024 done")
        return
    lib = host_timer()
    Hm = np.ascontiguousarray(c["H"])
    mask, flags, fg = np.zeros((H, W), np.uint8), np.zeros(len(feats), np.uint8), C.c_int(0)

    def host_us(reps):
        return lib.framediff_host_time_us(c["a"].ctypes.data, c["b"].ctypes.data, W, H, Hm.ctypes.data, c["flags"], c["threshold"], c["maxval"], mask.ctypes.data,
                                          len(feats), feats.ctypes.data, flags.ctypes.data, reps, C.byref(fg))
    print(f"library {framediff.lib_path()}  640x480, {len(feats)} features, median of {a.rounds} rounds; host = frame_diff_host, one thread, this repository's C++ (not OpenCV)")
    for n, reps in ((1, 50), (64, 5), (1024, 1)):
        for resident in (True, False):
            for want_mask in (True, False):
                if n == 1024 and not resident and want_mask and a.rounds > 3:
                    rounds = 3
                else:
                    rounds = a.rounds
                p = prepared(n, resident, want_mask)
                device_us(p, 2)
                host_us(1)
                dev, host = [], []
                for _ in range(rounds):
                    dev.append(device_us(p, reps))
                    host.append(host_us(3))
                r = p.results()[n - 1]
                assert r["n_foreground"] == want["n_foreground"] == fg.value and np.array_equal(r["flags"], want["flags"]) and np.array_equal(mask, want["mask"])
                d, h = statistics.median(dev), statistics.median(host)
                print(f"n = {n:4d}  {'device-resident' if resident else 'pageable':15s}  {'mask read back' if want_mask else 'flags only':14s}  "
                      f"{d:10.1f} us per call  {d / n:8.1f} us per pair  (min {min(dev) / n:8.1f})  host {h:8.1f} us per pair  ratio {h * n / d:7.1f}", flush=True)
                del p


if __name__ == "__main__":
    main()
