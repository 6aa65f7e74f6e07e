"""Times dsdtm_motion_step / dsdtm_motion_steps (libdsdtm_amd_motion.so) at 640x480 against the C restatement on one CPU thread.

    python tools/time_motion.py [--reps 200] [--out FILE]            # the table of profiles/r15_motion_mask.txt
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/time_motion.py --trace     # kernel-only times, a run of its own

Rows: one step with the image in host memory and in device memory, each with the mask read back and with the mask left on the
device (200 feature flags only); the batch entry at n = 16, 64, 256, 1024 with device images, flags only and with every mask read
back. Every call is synchronous (it ends in the library's wait), so a host clock around it is the call's time. Each shape is
pre-rolled before it is timed; medians and the 10th / 90th percentiles are reported. The baseline is tests/motion_restatement.c at
-O2 -ffp-contract=off on one thread of the same machine: a plain scalar C program, NOT OpenCV's vectorised median.
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from dsdtm_amd import motion  # noqa: E402
from tests import motion_cases as mc  # noqa: E402

W, H = 640, 480
HOMOGRAPHY = [1.0005, 0.001, -1.75, -0.001, 1.0005, 0.6, 1e-6, -1e-6, 1.0]


def _stats(samples):
    s = sorted(samples)
    return dict(median_us=1e6 * statistics.median(s), p10_us=1e6 * s[len(s) // 10], p90_us=1e6 * s[(9 * len(s)) // 10], reps=len(s))


def _timed(fn, reps, preroll):
    for _ in range(preroll):
        fn()
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        out.append(time.perf_counter() - t0)
    return _stats(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--out", default=None)
    ap.add_argument("--trace", action="store_true", help="a short run for rocprofv3 --kernel-trace: 20 single steps, 5 batches of 64")
    ap.add_argument("--batches", default="16,64,256,1024")
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "no GPU: this tool measures on the device and has no fallback"
    wd = mc.world("real")
    img = np.ascontiguousarray(mc.image_of(wd, 2))
    feats = np.random.default_rng(1).uniform([0, 0], [W - 1, H - 1], size=(200, 2)).astype(np.float32)
    dev = torch.from_numpy(img).cuda()
    torch.cuda.synchronize()
    ctx = motion.MotionContext(0)
    rows = {}
    model = motion.MotionModel(ctx, W, H)

    def one(image, **kw):            # a prepared n = 1 call: the C call alone is timed
        p = ctx.prepare([dict(model=model, image=image, H=HOMOGRAPHY, **kw)])

        def call():
            assert p.run_raw() == 0, ctx.last_error()
        return call
    single = {"step host image, mask read back": one(img), "step host image, 200 flags only": one(img, want_mask=False, features=feats),
              "step device image, mask read back": one(dev), "step device image, 200 flags only": one(dev, want_mask=False, features=feats)}
    if a.trace:
        for fn in single.values():
            for _ in range(5):
                fn()
        models = [motion.MotionModel(ctx, W, H) for _ in range(64)]
        batch = [dict(model=m, image=dev, H=HOMOGRAPHY, want_mask=False, features=feats) for m in models]
        for _ in range(5):
            ctx.steps(batch)
        print("trace run done")
        return
    # the CPU baseline: the C restatement, one thread
    lib = mc.c_twin(tempfile.mkdtemp(prefix="motion_twin_"))
    st = np.zeros((12, (W // 4) * (H // 4)), np.float32)
    lib.motion_model_init(st.ctypes.data, W, H)
    mask, scratch = np.zeros((H, W), np.uint8), np.zeros((H, W), np.uint8)
    Hc = np.ascontiguousarray(HOMOGRAPHY, np.float64)
    rows["C restatement -O2, one thread (median + model)"] = _timed(
        lambda: lib.motion_step(st.ctypes.data, W, H, img.ctypes.data, W, Hc.ctypes.data, mask.ctypes.data, W, scratch.ctypes.data, None, None),
        max(10, a.reps // 10), 3)
    rows["C restatement -O2, 5x5 median alone"] = _timed(lambda: lib.motion_median5(img.ctypes.data, W, H, W, scratch.ctypes.data), max(10, a.reps // 10), 3)
    for name, fn in single.items():
        rows[name] = _timed(fn, a.reps, 20)
    for n in [int(v) for v in a.batches.split(",") if v]:
        models = [motion.MotionModel(ctx, W, H) for _ in range(n)]
        for label, want_mask in (("200 flags each", False), ("every mask read back", True)):
            batch = [dict(model=m, image=dev, H=HOMOGRAPHY, want_mask=want_mask, features=feats) for m in models]
            prepared = ctx.prepare(batch)            # the descriptors are built once: the C call alone is timed

            def call():
                assert prepared.run_raw() == 0, ctx.last_error()
            r = _timed(call, max(5, a.reps // max(1, n // 4)), 3)
            r["per_model_us"] = r["median_us"] / n
            rows[f"steps n = {n}, device images, {label}"] = r
        for m in models:
            m.close()
    base = rows["C restatement -O2, one thread (median + model)"]["median_us"]
    lines = [f"{'row':<58} {'median us':>11} {'p10':>10} {'p90':>10} {'per model':>10} {'x CPU':>8}"]
    for name, r in rows.items():
        per = r.get("per_model_us", r["median_us"])
        lines.append(f"{name:<58} {r['median_us']:>11.1f} {r['p10_us']:>10.1f} {r['p90_us']:>10.1f} {per:>10.1f} {base / per:>8.2f}")
    text = "\n".join(lines)
    print(text)
    print(json.dumps(dict(tool="time_motion", width=W, height=H, rows=rows)))
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
