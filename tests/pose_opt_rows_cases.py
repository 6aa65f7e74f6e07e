"""Cases for the several-frames-per-wavefront pose refinement kernels (pose_opt_rows_kernel<2> / <4>, picked by
pose_opt_launch from 4096 / 8192 frames on): a fixed set of small problems, a frame -> problem layout that moves
every problem through every row of a wavefront, and the packed arrays of dsdtm_pose_optimization_batch_device with
poison behind every frame's feature count and guard frames behind the batch. Deterministic, numpy only; shared by
tests/test_pose_opt_rows_cpu.py (which holds the set to its conditions) and tests/test_pose_opt_rows_gpu.py.

The set: K = 512 problems of at most MAX_FEATURES = 48 features. Problems 0 .. N_RANDOM - 1 come from
synth.make_pose_problem(SEED_BASE + k) with 1..48 features and max_level, unused_frac, outlier_frac, seed_t, seed_w
drawn per problem from default_rng(DRAW_SEED); the last ten are planted (PLANTED names them, in order).
problems33() is a second, smaller set of problems with exactly 33 features (n_features == NULL runs).

Replaced seeds: none. (A problem whose two oracle forms disagree in an exact field, or on which the kernel and the
oracle disagree in one, is replaced only with the oracle's trace rows as evidence that the tested quantity lies within
summation noise of its limit; it is then listed here with that evidence.)"""
import ctypes

import numpy as np

from dsdtm_amd import capi, synth

K = 512
MAX_FEATURES = 48
SEED_BASE = 7000
DRAW_SEED = 20240
PLANTED = ("zero_features", "nothing_used", "evaluation_failure", "n1", "n16", "n17", "n32", "n33", "n48", "only_47")
N_RANDOM = K - len(PLANTED)
K33 = 64
SENTINEL = 0xA5                 # guard frames (and the summaries before a launch) are filled with this byte

_CACHE = {}


def planted_index(name):
    return N_RANDOM + PLANTED.index(name)


def _empty(P):
    return synth.PoseProblem(np.zeros((0, 3)), np.zeros((0, 3)), np.zeros(0, np.int32), np.zeros(0, np.uint8), P.T_seed, P.T_true)


def _planted():
    out = []
    base = synth.make_pose_problem(SEED_BASE + 900, n=20, max_level=2, unused_frac=0.3)
    out.append(_empty(base))                                                   # zero_features
    P = synth.make_pose_problem(SEED_BASE + 901, n=20, max_level=2, unused_frac=0.3)
    P.use = np.zeros_like(P.use)
    out.append(P)                                                              # nothing_used
    # one used map point exactly on the camera plane of an identity seed pose (as tests/test_pose_opt_gpu.py::test_edge_cases)
    P = synth.make_pose_problem(SEED_BASE + 902, n=20, max_level=2, unused_frac=0.3)
    i = int(np.nonzero(P.use)[0][0])
    P.p_world = P.p_world.copy()
    P.p_world[i] = [0.3, -0.2, 0.0]
    P.T_seed = np.ascontiguousarray(np.eye(4)[:3])
    out.append(P)                                                              # evaluation_failure
    for j, n in enumerate((1, 16, 17, 32, 33, 48)):                            # the row strides and one past them, all used
        out.append(synth.make_pose_problem(SEED_BASE + 910 + j, n=n, max_level=2, unused_frac=0.0))
    P = synth.make_pose_problem(SEED_BASE + 920, n=48, max_level=2, unused_frac=0.0)
    P.use = np.zeros_like(P.use)
    P.use[47] = 1                                                              # the last lane of the last trip, alone
    out.append(P)                                                              # only_47
    assert len(out) == len(PLANTED)
    return out


def problems():
    """The K problems (a cached list; do not modify)."""
    if "problems" not in _CACHE:
        rng = np.random.default_rng(DRAW_SEED)
        out = []
        for k in range(N_RANDOM):
            n = int(rng.integers(1, MAX_FEATURES + 1))
            kw = dict(max_level=int(rng.integers(0, 5)), unused_frac=float(rng.choice([0.0, 0.1, 0.5])),
                      outlier_frac=float(rng.choice([0.05, 0.3])), seed_t=float(rng.choice([0.03, 0.15])),
                      seed_w=float(rng.choice([0.02, 0.1])))
            out.append(synth.make_pose_problem(SEED_BASE + k, n=n, **kw))
        out += _planted()
        assert len(out) == K
        _CACHE["problems"] = out
    return _CACHE["problems"]


def problems33():
    """K33 problems of exactly 33 features with a mix of use bytes: with max_features = 33 and no n_features array one
    lane is live in the last trip of both row strides (16 and 32)."""
    if "problems33" not in _CACHE:
        rng = np.random.default_rng(DRAW_SEED + 1)
        out = []
        for k in range(K33):
            kw = dict(max_level=int(rng.integers(0, 5)), unused_frac=float(rng.choice([0.0, 0.1, 0.5])),
                      outlier_frac=float(rng.choice([0.05, 0.3])), seed_t=float(rng.choice([0.03, 0.15])),
                      seed_w=float(rng.choice([0.02, 0.1])))
            out.append(synth.make_pose_problem(SEED_BASE + 2000 + k, n=33, **kw))
        out[0].use[:] = 1
        out[1].use[:] = 0
        out[1].use[32] = 1                              # the one lane of the last trip, alone
        out[2].use[32] = 0
        _CACHE["problems33"] = out
    return _CACHE["problems33"]


def layout(n_frames, k=K):
    """frame -> problem. Within a run of k frames the problems step by 131 (coprime with k: a permutation); every further
    run is shifted by one, which moves a problem to the next row of its wavefront (k is a multiple of 4) and beside three
    other problems."""
    f = np.arange(n_frames, dtype=np.int64)
    return ((f * 131 + f // k) % k).astype(np.int64)


class Packed:
    """The arrays of dsdtm_pose_optimization_batch_device, every one with guard_frames frames behind frame n_frames - 1."""


def pack(problems, frame_to_problem, max_features, guard_frames=4, over_count=None):
    """Inputs: columns behind a frame's n_features (and the guard frames) are poisoned — NaN in bearing and p_world, 40
    in level, 1 in use. Outputs: residual_norm is -1, summary SENTINEL bytes; the guard frames of T_cur_w, summary and
    residual_norm are SENTINEL bytes. over_count = (problem index, count) sets n_features of that problem's frames to
    count (> max_features: the kernel clamps)."""
    f2p = np.asarray(frame_to_problem, np.int64)
    F, G, M, kp = len(f2p), guard_frames, max_features, len(problems)
    b = np.full((kp, M, 3), np.nan); pw = np.full((kp, M, 3), np.nan)
    lv = np.full((kp, M), 40, np.int32); us = np.ones((kp, M), np.uint8)
    nf = np.zeros(kp, np.int32); T = np.zeros((kp, 12))
    for k, P in enumerate(problems):
        n = len(P.use)
        assert n <= M, (k, n, M)
        b[k, :n] = P.bearing; pw[k, :n] = P.p_world; lv[k, :n] = P.level; us[k, :n] = P.use
        nf[k] = n; T[k] = np.asarray(P.T_seed, np.float64).reshape(12)
    if over_count is not None:
        assert nf[over_count[0]] == M and over_count[1] > M
        nf[over_count[0]] = over_count[1]
    pk = Packed()
    pk.n_frames, pk.max_features, pk.guard_frames, pk.frame_to_problem = F, M, G, f2p
    pk.bearing = np.full((F + G, M, 3), np.nan); pk.bearing[:F] = b[f2p]
    pk.p_world = np.full((F + G, M, 3), np.nan); pk.p_world[:F] = pw[f2p]
    pk.level = np.full((F + G, M), 40, np.int32); pk.level[:F] = lv[f2p]
    pk.use = np.ones((F + G, M), np.uint8); pk.use[:F] = us[f2p]
    pk.n_features = np.full(F + G, M, np.int32); pk.n_features[:F] = nf[f2p]
    sent = np.frombuffer(bytes([SENTINEL]) * 8, np.float64)[0]
    pk.T_cur_w = np.full((F + G, 12), sent); pk.T_cur_w[:F] = T[f2p]
    pk.residual_norm = np.full((F + G, M), sent); pk.residual_norm[:F] = -1.0
    pk.summary = np.full((F + G, ctypes.sizeof(capi.PoseOptSummary)), SENTINEL, np.uint8)
    return pk
