"""Wall per dsdtm_klt_steps call at 640x480 for n = 1, 64, 1024 models: a pageable image against a device image, correspondences read
back against not read back; beside it klt_step_host (tools/klt_host_timer.cpp, the repository's own C++ on one host thread, not OpenCV;
it has no homography). Wall times of whole calls: no kernel-only time is taken here (that needs a profiler pass of its own).

    python tools/time_klt.py [--reps 20] [--n 1 64 1024] > profiles/r24_klt.txt
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
from dsdtm_amd import klt  # noqa: E402


def frame(w, h, shift):
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    u = x - shift
    return (128.0 + 45.0 * np.sin(u * 0.21 + y * 0.05) + 40.0 * np.cos(y * 0.17 - u * 0.07) + 30.0 * np.sin(u * 0.09) * np.cos(y * 0.11)).astype(np.uint8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--n", type=int, nargs="+", default=[1, 64, 1024])
    a = ap.parse_args()
    import torch
    w, h = 640, 480
    imgs = [frame(w, h, 0), frame(w, h, 3)]
    dev = [torch.from_numpy(i).cuda() for i in imgs]
    ctx = klt.KltContext(0)
    print(f"dsdtm_klt_steps, {w}x{h}, 361 grid points, {a.reps} calls per row (after 3 warm-up calls), wall per call")
    for n in a.n:
        models = [klt.KltModel(ctx, w, h) for _ in range(n)]
        for image_kind, pair in (("pageable", imgs), ("device", dev)):
            for want in (False, True):
                steps = [[dict(model=m, image=pair[k], want=want) for m in models] for k in (0, 1)]
                for k in range(3):
                    ctx.steps(steps[k % 2])
                t0 = time.perf_counter()
                for k in range(a.reps):
                    r = ctx.steps(steps[(k + 1) % 2])
                dt = (time.perf_counter() - t0) / a.reps * 1e6
                print(f"n = {n:5d}  image {image_kind:8s}  correspondences {'read back' if want else 'left on the device'}: {dt:10.1f} us per call, "
                      f"{dt / n:8.1f} us per model  (source {r[0]['source']}, {r[0]['n_tracked']} tracked, {r[0]['n_inliers']} inliers)", flush=True)
        for m in models:
            m.close()
    ctx.close()
    exe = os.path.join(tempfile.mkdtemp(), "klt_host_timer")
    subprocess.run([os.environ.get("CXX", "g++"), "-O2", "-std=c++17", "-ffp-contract=off", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tools", "klt_host_timer.cpp"), "-o", exe], check=True)
    print(subprocess.run([exe, str(a.reps)], capture_output=True, text=True, check=True).stdout.strip())
    print("(the Python binding builds n descs per call; its share is in the wall time of the large n rows)")


if __name__ == "__main__":
    main()
