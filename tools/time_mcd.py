"""Times the whole MCDWrapper::Run on the device (dsdtm_mcd_steps, libdsdtm_amd_mcd.so) at 640x480 against the path a caller had before
it — dsdtm_motion_steps with every mask read back, then mcd_box_host (dsdtm_amd/host/dsdtm_mcd_host.hpp) per mask on ONE host thread —
and against mcd_box_host alone.

    python tools/time_mcd.py [--reps 100] [--batches 1,64,1024] [--out profiles/r23_mcd.txt]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/time_mcd.py --trace      # kernel-only times, a run of its own

Setup: that of tools/time_motion.py (profiles/r15_motion_mask.txt) — the real 640x480 image, device images, 200 features — with one
change: every timed call sees the frame with the bright block pasted in, and an untimed call on the plain frame goes before it, so
that detect_img holds a blob each time (a model fed the same frame over and over learns it and the mask goes empty). The three paths
alternate in one process on the same models' worth of work. Every call is synchronous; medians, 10th and 90th percentiles.
The baseline is THIS REPOSITORY'S OWN C++ (flood fill, a border walk per candidate), not OpenCV's findContours.
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

from dsdtm_amd import mcd, motion  # noqa: E402
from tests import mcd_cases as cases  # noqa: E402
from tests import motion_cases as mc  # noqa: E402

W, H = 640, 480
HOMOGRAPHY = [1.0005, 0.001, -1.75, -0.001, 1.0005, 0.6, 1e-6, -1e-6, 1.0]


def _stats(samples):
    s = sorted(samples)
    return dict(median_us=1e6 * statistics.median(s), p10_us=1e6 * s[len(s) // 10], p90_us=1e6 * s[(9 * len(s)) // 10], reps=len(s))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--out", default=None)
    ap.add_argument("--trace", action="store_true", help="a short run for rocprofv3 --kernel-trace: 10 calls at n = 1 and 3 at n = 64")
    ap.add_argument("--batches", default="1,64,1024")
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "no GPU: this tool measures on the device and has no fallback"
    wd = mc.world("real")
    plain, block = (torch.from_numpy(np.ascontiguousarray(mc.image_of(wd, s))).cuda() for s in (0, 2))
    torch.cuda.synchronize()
    feats = np.random.default_rng(1).uniform([0, 0], [W - 1, H - 1], size=(200, 2)).astype(np.float32)
    box_host = cases.host_function(tempfile.mkdtemp(prefix="mcd_host_")).mcd_box_host_c
    cctx, mctx = mcd.McdContext(0), motion.MotionContext(0)
    rows, text = {}, []
    for n in [int(v) for v in a.batches.split(",") if v]:
        cm = [mcd.McdModel(cctx, W, H) for _ in range(n)]
        mm = [motion.MotionModel(mctx, W, H) for _ in range(n)]
        new = {img: cctx.prepare([dict(model=m, image=t, H=HOMOGRAPHY, want_mask=False, features=feats) for m in cm]) for img, t in (("plain", plain), ("block", block))}
        old = {img: mctx.prepare([dict(model=m, image=t, H=HOMOGRAPHY, want_mask=True, features=feats) for m in mm]) for img, t in (("plain", plain), ("block", block))}
        masks = [o[0] for o in old["block"].outs]

        def host_boxes():
            out = []
            for mask in masks:
                r = cases.run_c(box_host, mask)
                out.append((r["box"], r["area2"], r["n_components"]))
            return out

        def run_new():
            assert new["block"].run_raw() == 0, cctx.last_error()

        def run_old():
            assert old["block"].run_raw() == 0, mctx.last_error()
            host_boxes()
        if a.trace:
            for _ in range(10 if n == 1 else 3):
                assert new["plain"].run_raw() == 0 and new["block"].run_raw() == 0
            continue
        samples = {"new": [], "old": [], "host": []}
        reps = max(5, a.reps // max(1, n // 8))
        for k in range(reps + 3):
            assert new["plain"].run_raw() == 0 and old["plain"].run_raw() == 0
            for name, fn in (("new", run_new), ("old", run_old), ("host", host_boxes)):
                t0 = time.perf_counter()
                fn()
                if k >= 3:
                    samples[name].append(time.perf_counter() - t0)
        got = [(r["box"], r["area2"], r["n_components"]) for r in new["block"].results()]
        assert got == host_boxes(), "the device and mcd_box_host disagree"
        for name, label in (("new", "dsdtm_mcd_steps, 200 flags + box each"), ("old", "dsdtm_motion_steps + masks back + mcd_box_host"), ("host", "mcd_box_host alone, one thread")):
            r = _stats(samples[name])
            r["per_model_us"] = r["median_us"] / n
            rows[f"n = {n}: {label}"] = r
        rows[f"n = {n}: box"] = dict(box=got[0][0], area2=got[0][1], n_components=got[0][2])
        for m in cm + mm:
            m.close()
    if a.trace:
        print("trace run done")
        return
    text.append(f"{'row':<62} {'median us':>11} {'p10':>10} {'p90':>10} {'per model':>10}")
    for name, r in rows.items():
        if "median_us" in r:
            text.append(f"{name:<62} {r['median_us']:>11.1f} {r['p10_us']:>10.1f} {r['p90_us']:>10.1f} {r['per_model_us']:>10.1f}")
        else:
            text.append(f"{name:<62} {json.dumps(r)}")
    print("\n".join(text))
    print(json.dumps(dict(tool="time_mcd", width=W, height=H, rows=rows)))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(text) + "\n")


if __name__ == "__main__":
    main()
