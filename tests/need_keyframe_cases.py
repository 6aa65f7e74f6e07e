"""Cases of Tracking::NeedKeyframe shared by tests/test_need_keyframe_cpu.py (the restatement against hand-computed answers)
and tests/test_need_keyframe_gpu.py (the device entry and the host function against the restatement): the exact-threshold
cases, whose inputs are exactly representable, and seeded random trackers of given shapes."""
from types import SimpleNamespace

import numpy as np

from dsdtm_amd import keyframe_decision as K
from dsdtm_amd import synth

CAM = SimpleNamespace(fx=512.0, fy=512.0, cx=320.0, cy=240.0, f=512.0, width=640, height=480)
I34 = np.hstack([np.eye(3), np.zeros((3, 1))])


def pose(tx=0.0, ty=0.0, tz=0.0):
    T = I34.copy()
    T[:, 3] = (tx, ty, tz)
    return T


def make(T_cur=None, T_kf=None, n_valid=100, cur_p=None, cur_bad=None, kf_p=None, kf_bad=None, lkf=None, params=None, cam=CAM):
    """A tracker on which no rule fires unless an argument makes one: identity poses, more valid points than K1's window."""
    return dict(cam=cam, T_cur=I34.copy() if T_cur is None else np.asarray(T_cur, np.float64).reshape(3, 4),
                T_kf=I34.copy() if T_kf is None else np.asarray(T_kf, np.float64).reshape(3, 4), n_valid=int(n_valid),
                cur_p=np.asarray([[0.0, 0.0, 2.0]] * 3 if cur_p is None else cur_p, np.float64).reshape(-1, 3),
                cur_bad=None if cur_bad is None else np.asarray(cur_bad, np.uint8),
                kf_p=np.asarray([[0.0, 0.0, 1.0]] * 3 if kf_p is None else kf_p, np.float64).reshape(-1, 3),
                kf_bad=None if kf_bad is None else np.asarray(kf_bad, np.uint8),
                lkf=np.asarray(np.zeros((0, 3)) if lkf is None else lkf, np.float64).reshape(-1, 3),
                params=params or K.KeyframeParams())


def run_reference(c):
    return K.need_keyframe_reference(c["cam"], c["T_cur"], c["T_kf"], c["n_valid"], c["cur_p"], c["cur_bad"], c["kf_p"],
                                     c["kf_bad"], c["lkf"], c["params"])


def desc_of(c):
    """The case as capi.KeyframeCall wants a tracker."""
    return dict(T_cur_w=c["T_cur"], T_kf_w=c["T_kf"], n_valid=c["n_valid"], cur_p_world=c["cur_p"], cur_bad=c["cur_bad"],
                kf_p_world=c["kf_p"], kf_bad=c["kf_bad"], local_kf_centre=c["lkf"])


# ---- exact-threshold cases (every quantity below is exactly representable; test_need_keyframe_cpu.py checks the claims) ----
def _k2_at_threshold():
    kf = [[(i - 15) / 64.0, (i % 5 - 2) / 64.0, 1.0] for i in range(35)]
    return make(T_cur=pose(40.0 / 512.0), kf_p=kf, params=K.KeyframeParams(min_trans=10.0))


def _k2_above_threshold():
    # 512 * 2^-52 = 2^-43 = two ulps of 360: the step survives the addition of cx
    kf = [[0.0, (i % 5 - 2) / 64.0, 1.0] for i in range(35)]
    return make(T_cur=pose(40.0 / 512.0 + 2.0 ** -52), kf_p=kf, params=K.KeyframeParams(min_trans=10.0))


def _k3_trans_equal():
    return make(T_cur=pose(0.125), kf_p=[[0.0, 0.0, 4.0]] * 3, params=K.KeyframeParams(min_rot=1.0, min_trans=0.125))


def _k4(centre):
    cur = [[0.0, 0.0, 2.0], [0.5, 0.25, 2.0], [-0.5, 0.125, 2.0], [0.25, -0.5, 2.0], [0.0, 0.5, 2.0]]
    return make(cur_p=cur, lkf=[centre])


def _k2_31_stop():
    kf = [[0.0, 0.0, 1.0 / (i + 1)] for i in range(31)] + [[0.0, 0.0, 2.0 ** -12]] * 9
    return make(T_cur=pose(1.0 / 512.0), kf_p=kf, params=K.KeyframeParams(min_trans=1.0, min_px_median=1e6))


def small_then_huge(n_small, n=40):
    """n keyframe points: n_small displaced by exactly 8 px, the rest by exactly 4096 px."""
    kf = [[0.0, 0.0, 1.0]] * n_small + [[0.0, 0.0, 2.0 ** -9]] * (n - n_small)
    return make(T_cur=pose(8.0 / 512.0), kf_p=kf, params=K.KeyframeParams(min_trans=1.0))


EXACT = {
    "k2_at_threshold": _k2_at_threshold,
    "k2_above_threshold": _k2_above_threshold,
    "k3_trans_equal": _k3_trans_equal,
    "k4_equal": lambda: _k4([4.0, 3.2, 5.2]),
    "k4_fabs_quirk": lambda: _k4([-4.0, 3.2, 5.2]),
    "k2_31_stop": _k2_31_stop,
    "small_then_huge_20": lambda: small_then_huge(20),
    "k1_low_edge": lambda: make(n_valid=30),
    "k1_high_edge": lambda: make(n_valid=50),
    "k1_below": lambda: make(n_valid=29),
    "k1_above": lambda: make(n_valid=51),
    "empty_lists": lambda: make(kf_p=np.zeros((0, 3)), cur_p=np.zeros((0, 3)), lkf=[[4.0, 3.2, 5.2]]),
}


# ---- seeded random trackers ---------------------------------------------------------------------------------------------
def _to_world(T34, pc):
    R, t = T34[:, :3], T34[:, 3]
    return (np.asarray(pc, np.float64) - t) @ R            # R^T (p - t), row-wise


def random_case(seed, n_cur, n_kf, n_lkf, depth="positive", bad="some", fire=None, motion=0.02, n_valid=100):
    """depth: positive (0.5 .. 6 m in front of the current camera) / negative / mixed / equal / duplicates; bad: none / some /
    all (both lists); fire: index of the one local keyframe that fires K4, or None (the others lie behind the camera plane of
    the rule: their x is negative)."""
    rng = np.random.default_rng(seed)
    T_kf = synth.se3_exp(np.concatenate([rng.uniform(-1, 1, 3), rng.uniform(-0.3, 0.3, 3)]))[:3]
    d = synth.se3_exp(np.concatenate([rng.uniform(-motion, motion, 3), rng.uniform(-motion, motion, 3)]))
    T_cur = (d @ np.vstack([T_kf, [0, 0, 0, 1]]))[:3]

    def points(n):
        if depth == "equal":
            z = np.full(n, 2.5)
        elif depth == "duplicates":
            z = rng.choice([0.75, 1.5, 1.5, 3.0], n)
        else:
            z = rng.uniform(0.5, 6.0, n)
            if depth == "negative":
                z = -z
            elif depth == "mixed":
                z = z * rng.choice([-1.0, 1.0], n)
        pc = np.stack([rng.uniform(-0.5, 0.5, n) * z, rng.uniform(-0.4, 0.4, n) * z, z], 1)
        return _to_world(T_cur, pc)

    def flags(n):
        if bad == "none":
            return None
        return np.ones(n, np.uint8) if bad == "all" else (rng.uniform(size=n) < 0.2).astype(np.uint8)

    c = make(T_cur=T_cur, T_kf=T_kf, n_valid=n_valid, cur_p=points(n_cur), cur_bad=flags(n_cur), kf_p=points(n_kf), kf_bad=flags(n_kf),
             lkf=np.zeros((n_lkf, 3)))
    m = run_reference(c)["median_depth"]
    lk = np.stack([-rng.uniform(0.5, 2.0, n_lkf) * max(1.0, m * m), rng.uniform(-1, 1, n_lkf), rng.uniform(-1, 1, n_lkf)], 1)
    if fire is not None and n_lkf:
        lk[fire] = (1.5 * m * m, 1.25 * m * m, 2.0 * m * m)
    c["lkf"] = _to_world(T_cur, lk).reshape(-1, 3)
    return c


def margins(c, r):
    """Relative distance of every measured quantity from the threshold it is compared with (the ones the case does not sit on
    exactly): a random case must keep all of them >= 1e-6, or a rounding difference could flip a rule."""
    p = c["params"]
    out = []
    if r["n_px"]:
        out.append(abs(r["median_px"] - p.min_px_median) / p.min_px_median)
    out.append(abs(r["rot"] - p.min_rot) / p.min_rot)
    out.append(abs(r["trans"] - p.min_trans) / p.min_trans)
    if r["n_depth"]:
        m = r["median_depth"]
        Tc = [float(v) for v in c["T_cur"].reshape(12)]
        last = len(c["lkf"]) if r["svo_kf"] < 0 else r["svo_kf"] + 1
        for j in range(last):
            cc = K.transform(Tc, [float(v) for v in c["lkf"][j]])
            for v, k in zip(cc, (1.0, 0.8, 1.3)):
                out.append(abs(v / m - k * m) / max(abs(k * m), 1e-300))
    return out


# ---- the compiled driver (tests/need_keyframe_host/driver.cpp): need_keyframe_host and the device entry on the same cases ----
def write_cases(path, cs):
    import struct
    with open(path, "wb") as f:
        f.write(struct.pack("<i4f", len(cs), CAM.fx, CAM.fy, CAM.cx, CAM.cy))
        for c in cs:
            p = c["params"]
            f.write(struct.pack("<3i3d", p.min_valid, p.max_valid, p.px_samples, p.min_px_median, p.min_rot, p.min_trans))
            f.write(np.ascontiguousarray(c["T_cur"], "<f8").tobytes() + np.ascontiguousarray(c["T_kf"], "<f8").tobytes())
            f.write(struct.pack("<6i", c["n_valid"], len(c["cur_p"]), len(c["kf_p"]), len(c["lkf"]),
                                int(c["cur_bad"] is not None), int(c["kf_bad"] is not None)))
            for pts, bad in ((c["cur_p"], c["cur_bad"]), (c["kf_p"], c["kf_bad"])):
                f.write(np.ascontiguousarray(pts, "<f8").tobytes())
                f.write((np.zeros(len(pts), np.uint8) if bad is None else np.ascontiguousarray(bad, np.uint8)).tobytes())
            f.write(np.ascontiguousarray(c["lkf"], "<f8").tobytes())


INT_FIELDS = ("need", "reason", "rule_mask", "undefined", "n_px", "n_depth", "svo_kf")
FLOAT_FIELDS = ("median_px", "rot", "trans", "min_depth", "median_depth")


def run_driver(tmp_path, cs, host_only=False):
    """{"host": [verdict dicts], "device": [...]} as the compiled driver prints them (17 digits: the doubles round-trip)."""
    import os
    import subprocess
    from dsdtm_amd import capi
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe, lib = str(tmp_path / "need_keyframe_driver"), capi.keyframe_lib_path()
    subprocess.run(["g++", "-O2", "-std=c++14", "-Wall", "-ffp-contract=off", "-o", exe, os.path.join(root, "tests", "need_keyframe_host", "driver.cpp"),
                    lib, "-Wl,-rpath," + os.path.dirname(lib), "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib", "-lamdhip64"], check=True)
    write_cases(tmp_path / "cases.bin", cs)
    out = subprocess.run([exe, str(tmp_path / "cases.bin")] + (["host"] if host_only else []), capture_output=True, text=True, check=True).stdout
    res = {"host": [], "device": []}
    for line in out.strip().split("\n"):
        t = line.split()
        assert int(t[1]) == len(res[t[0]])
        res[t[0]].append(dict(zip(INT_FIELDS + FLOAT_FIELDS, [int(v) for v in t[2:9]] + [float(v) for v in t[9:14]])))
    return res


def assert_same_verdict(got, want, what, rtol=1e-9, exact_medians=True):
    """The acceptance check: the integer fields equal; the floating ones within rtol (relative); the two medians (selected, not
    computed: a selection hands the element through unchanged) bit-equal when both sides selected from the same computed values."""
    for k in INT_FIELDS:
        assert got[k] == want[k], (what, k, got[k], want[k])
    if want["undefined"]:
        return
    for k in FLOAT_FIELDS:
        assert abs(got[k] - want[k]) <= rtol * abs(want[k]), (what, k, got[k], want[k])
    if exact_medians:
        assert got["median_px"] == want["median_px"] and got["median_depth"] == want["median_depth"], (what, got, want)
