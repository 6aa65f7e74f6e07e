"""Builds the HIP library in-tree with hipcc for gfx950 (cross-compiles without a GPU).

    python dsdtm_amd/csrc/build.py            # the RELEASE library  libdsdtm_amd.so       (the product)
    python dsdtm_amd/csrc/build.py --diag     # the DIAGNOSTIC build libdsdtm_amd_diag.so  (tools/, diag-marked tests)
    python dsdtm_amd/csrc/build.py --all      # both, and the add-on libraries (the ADDONS table)
    ... [--force] [--define X=1 ...] [--flag F ...]   (extra flags: experiments, see below)

RELEASE (default): exports exactly the symbols include/dsdtm_amd.h declares (linker version script exports.map), reads no
environment variable, has no dsdtm_debug_* entry, and does not contain what only the diagnostic build reaches (the stamps
instantiation of the register kernel, selftest.hip, the two-kernel FindMatchDirect path). bench.py, __graft_entry__.smoke()
and every parity test load this one. DIAG (-DDSDTM_DIAG): the same sources with the switches of kernels.h as process-wide
variables (DSDTM_* environment, dsdtm_debug_set_option), the dsdtm_debug_* entries and those kernels; loaded by tools/ and
by the tests marked `diag` (fault injection: a team member that stays away, the epoch wrap, the fused kernels held to the
paths they replaced).

Every source is compiled to its own object under csrc/build/ (only when it or a header is newer; in parallel; objects are
keyed by the flag set), then linked: a change to one kernel file recompiles that file only. The flag set a library was
linked from is recorded beside it (<lib>.tag): a request for another flag set relinks even when every object is fresh, so an
experiment build (--define / --flag) can never be mistaken for the default one. The add-on libraries (the ADDONS table) go
through the same routine, with the release flags.
"""
import argparse
import concurrent.futures
import hashlib
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
SOURCES = ["api.cpp", "api_track.cpp", "api_local_ba.cpp",   # the host side, over api_internal.h
           "sparse_align.hip", "align2d.hip", "pyrdown.hip", "warp.hip", "match.hip", "detect.hip", "pose_opt.hip", "track.hip", "local_ba.hip", "rgbd.hip"]
DIAG_SOURCES = ["selftest.hip"]                      # diagnostic build only
HEADERS = ["api_internal.h", "kernels.h", "device_math.h", "warp_body.h", "align2d_body.h", "match_body.h", "pose_math.h", "exports.map", os.path.join("..", "..", "include", "dsdtm_amd.h")]
OUT_KEYFRAME = os.path.join(HERE, "libdsdtm_amd_keyframe.so")
OUT_MOTION = os.path.join(HERE, "libdsdtm_amd_motion.so")
_INC = os.path.join("..", "..", "include")
# The add-on libraries: name -> (sources, headers, output). Each has sources and headers of its own (the host scaffold addon_host.h is
# shared among them), so that libdsdtm_amd.so, its symbols and its source hash, is untouched by them; built with the release flags by
# build_all() and --all. A new add-on is a new row.
ADDONS = {
    # include/dsdtm_amd_keyframe.h: Tracking::NeedKeyframe for n trackers
    "keyframe": (["keyframe_api.cpp", "keyframe.hip"],
                 ["keyframe.h", "addon_host.h", "device_math.h", "pose_math.h", "exports.map", os.path.join(_INC, "dsdtm_amd_keyframe.h"),
                  os.path.join(_INC, "dsdtm_amd.h")], OUT_KEYFRAME),
    # include/dsdtm_amd_motion.h: the moving-object mask of Tracking::MotionRemoval
    "motion": (["motion_api.cpp", "motion.hip"],
               ["motion_api_body.h", "motion.h", "addon_host.h", "exports.map", os.path.join(_INC, "dsdtm_amd_motion.h"), os.path.join(_INC, "dsdtm_amd.h")], OUT_MOTION),
    # include/dsdtm_amd_homography.h: the RANSAC homography that the motion step takes as an argument, for n trackers
    "homography": (["homography_api.cpp", "homography.hip"],
                   ["homography.h", "addon_host.h", "exports.map", os.path.join(_INC, "dsdtm_amd_homography.h"), os.path.join(_INC, "dsdtm_amd.h")],
                   os.path.join(HERE, "libdsdtm_amd_homography.so")),
    # include/dsdtm_amd_localmap.h: the device-resident map and the selection of Tracking::UpdateLocalMap / GetCloseKeyFrames
    "localmap": (["localmap_api.cpp", "localmap.hip"],
                 ["localmap.h", "addon_host.h", "exports.map", os.path.join(_INC, "dsdtm_amd_localmap.h"), os.path.join(_INC, "dsdtm_amd.h")],
                 os.path.join(HERE, "libdsdtm_amd_localmap.so")),
    # include/dsdtm_amd_trackmap.h: the resident track map and dsdtm_track_desc's local-map columns (the selection is localmap.hip's)
    "trackmap": (["trackmap_api.cpp", "trackmap.hip", "localmap.hip"],
                 ["trackmap_api_body.h", "trackmap.h", "localmap.h", "addon_host.h", "exports.map", os.path.join(_INC, "dsdtm_amd_trackmap.h"),
                  os.path.join(_INC, "dsdtm_amd_localmap.h"), os.path.join(_INC, "dsdtm_amd.h")],
                 os.path.join(HERE, "libdsdtm_amd_trackmap.so")),
    # include/dsdtm_amd_mapping.h: the same resident map (trackmap_api_body.h compiled under the dsdtm_mapping_* names) and the mapping
    # thread's covisibility list, local-BA window and commit
    "mapping": (["mapping_api.cpp", "mapping.hip", "trackmap.hip", "localmap.hip"],
                ["mapping.h", "mapping_api_body.h", "trackmap_api_body.h", "trackmap.h", "localmap.h", "addon_host.h", "exports.map", os.path.join(_INC, "dsdtm_amd_mapping.h"),
                 os.path.join(_INC, "dsdtm_amd_trackmap.h"), os.path.join(_INC, "dsdtm_amd_localmap.h"), os.path.join(_INC, "dsdtm_amd.h")],
                os.path.join(HERE, "libdsdtm_amd_mapping.so")),
    # include/dsdtm_amd_newkf.h: the walk and the lift of Tracking::CraeteKeyframe, from the per-cell corners to the keyframe's columns
    "newkf": (["newkf_api.cpp", "newkf.hip"],
              ["newkf.h", "addon_host.h", "exports.map", os.path.join(_INC, "dsdtm_amd_newkf.h"), os.path.join(_INC, "dsdtm_amd.h")],
              os.path.join(HERE, "libdsdtm_amd_newkf.so")),
    # include/dsdtm_amd_slam.h: the same resident map and the mapping entries (both bodies compiled under the dsdtm_slam_* names) and a
    # tracked frame's effects on the map and the gather of the keyframe decision on it (aftertrack.hip; keyframe.hip is linked as it is)
    "slam": (["slam_api.cpp", "aftertrack.hip", "mapping.hip", "trackmap.hip", "localmap.hip", "keyframe.hip"],
             ["aftertrack.h", "mapping.h", "mapping_api_body.h", "trackmap_api_body.h", "trackmap.h", "localmap.h", "keyframe.h", "addon_host.h",
              "device_math.h", "pose_math.h", "exports.map", os.path.join(_INC, "dsdtm_amd_slam.h"), os.path.join(_INC, "dsdtm_amd_mapping.h"),
              os.path.join(_INC, "dsdtm_amd_trackmap.h"), os.path.join(_INC, "dsdtm_amd_localmap.h"), os.path.join(_INC, "dsdtm_amd_keyframe.h"),
              os.path.join(_INC, "dsdtm_amd.h")],
             os.path.join(HERE, "libdsdtm_amd_slam.so")),
    # include/dsdtm_amd_undistort.h: cv::undistort of raw gray / depth frames and Frame::UndistortFeatures, in front of dsdtm_frame_prefetch
    "undistort": (["undistort_api.cpp", "undistort.hip"],
                  ["undistort.h", "addon_host.h", "exports.map", os.path.join(_INC, "dsdtm_amd_undistort.h"), os.path.join(_INC, "dsdtm_amd.h")],
                  os.path.join(HERE, "libdsdtm_amd_undistort.so")),
}
# Add-ons that came after the nine above: the same kind of row, built by the same routine and by build_all() / --all. (They stand in a
# table of their own because tests/test_undistort_cpu.py holds list(ADDONS) to those nine names.)
MORE_ADDONS = {
    # include/dsdtm_amd_mcd.h: the whole MCDWrapper::Run — the motion models and step (motion_api_body.h compiled under the dsdtm_mcd_* names;
    # motion.hip is linked as it is) and the contour box behind them (contour.hip)
    "mcd": (["mcd_api.cpp", "contour.hip", "motion.hip"],
            ["contour.h", "motion_api_body.h", "motion.h", "addon_host.h", "exports.map", os.path.join(_INC, "dsdtm_amd_mcd.h"),
             os.path.join(_INC, "dsdtm_amd_motion.h"), os.path.join(_INC, "dsdtm_amd.h")],
            os.path.join(HERE, "libdsdtm_amd_mcd.so")),
    # include/dsdtm_amd_klt.h: KLTWrapper::RunTrack — the grid's pyramidal Lucas-Kanade flow (klt.hip) and the H of the survivors
    # (homography.hip and pyrdown.hip are linked as they are)
    "klt": (["klt_api.cpp", "klt.hip", "homography.hip", "pyrdown.hip"],
            ["klt.h", "homography.h", "kernels.h", "addon_host.h", "exports.map", os.path.join(_INC, "dsdtm_amd_klt.h"),
             os.path.join(_INC, "dsdtm_amd_homography.h"), os.path.join(_INC, "dsdtm_amd.h")],
            os.path.join(HERE, "libdsdtm_amd_klt.so")),
    # include/dsdtm_amd_framediff.h: Moving_Detecter::Mod_FrameDiff — warp, difference, threshold, open, dilate and the feature test
    # (F1, the inverse of H, is the host header's function: one definition for the library and the host path)
    "framediff": (["framediff_api.cpp", "framediff.hip"],
                  ["framediff.h", "addon_host.h", "exports.map", os.path.join("..", "host", "dsdtm_framediff_host.hpp"),
                   os.path.join(_INC, "dsdtm_amd_framediff.h"), os.path.join(_INC, "dsdtm_amd.h")],
                  os.path.join(HERE, "libdsdtm_amd_framediff.so")),
    # include/dsdtm_amd_rarsac.h: Rarsac_base::RejectFundamental — the grid-guided RANSAC for the fundamental matrix, lane = hypothesis
    # (R1, the bin of a point, is the host header's function: one definition for the library and the host path)
    "rarsac": (["rarsac_api.cpp", "rarsac.hip"],
               ["rarsac.h", "addon_host.h", "exports.map", os.path.join("..", "host", "dsdtm_rarsac_host.hpp"),
                os.path.join(_INC, "dsdtm_amd_rarsac.h"), os.path.join(_INC, "dsdtm_amd.h")],
               os.path.join(HERE, "libdsdtm_amd_rarsac.so")),
    # include/dsdtm_amd_clahe.h: cv::CLAHE(3.0, 8x8) of the reference's drivers — per-tile tables, then the interpolation
    # (E1 and E2, the geometry of a frame, are the host header's function: one definition for the library and the host path)
    "clahe": (["clahe_api.cpp", "clahe.hip"],
              ["clahe.h", "addon_host.h", "exports.map", os.path.join("..", "host", "dsdtm_clahe_host.hpp"),
               os.path.join(_INC, "dsdtm_amd_clahe.h"), os.path.join(_INC, "dsdtm_amd.h")],
              os.path.join(HERE, "libdsdtm_amd_clahe.so")),
}
OUT = os.path.join(HERE, "libdsdtm_amd.so")
OUT_DIAG = os.path.join(HERE, "libdsdtm_amd_diag.so")
TAG = OUT + ".tag"
OBJ_DIR = os.path.join(HERE, "build")
DIAG_DEFINE = "-DDSDTM_DIAG=1"


def out_path(diag=False):
    return OUT_DIAG if diag else OUT


def _sources(diag):
    return SOURCES + (DIAG_SOURCES if diag else [])


def _flags(extra, diag=False):
    return ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-fno-gpu-rdc", *([DIAG_DEFINE] if diag else []), *extra]


def _tag(flags):
    return hashlib.sha1(" ".join(flags).encode()).hexdigest()[:8]


def _obj(src, flags):
    return os.path.join(OBJ_DIR, f"{os.path.splitext(src)[0]}.{_tag(flags)}.o")


def source_sha(extra=(), diag=False):
    """sha256 (16 hex digits) over the library's sources, headers and compiler flags: what a profile is tied to besides
    the hash of the binary it ran with (hipcc's objects are not reproducible byte for byte, the sources are)."""
    h = hashlib.sha256(" ".join(_flags(list(extra), diag)).encode())
    for f in sorted(_sources(diag) + HEADERS):
        with open(os.path.join(HERE, f), "rb") as fh:
            h.update(os.path.basename(f).encode() + b"\0" + fh.read())
    return h.hexdigest()[:16]


def _linked_tag(out):
    try:
        with open(out + ".tag") as f:
            return f.read().strip()
    except OSError:
        return None


def _stale(target, deps):
    if not os.path.exists(target):
        return True
    t = os.path.getmtime(target)
    return any(os.path.getmtime(d) > t for d in deps)


def _plan(sources, headers, flags):
    """(object, what it depends on) per source."""
    hdrs = [os.path.join(HERE, h) for h in headers] + [os.path.abspath(__file__)]
    return [(_obj(s, flags), [os.path.join(HERE, s)] + hdrs) for s in sources]


def _needs(sources, headers, out, flags):
    plan = _plan(sources, headers, flags)
    # (the objects first: one that is missing is stale, and has no time to hold the library's against)
    return (any(_stale(o, deps) for o, deps in plan) or _linked_tag(out) != _tag(flags) or _stale(out, [o for o, _ in plan]))


def _make(sources, headers, out, flags, force, verbose):
    """THE compile-and-link routine of every library here: each stale source to its own object (in parallel), then, if anything was
    compiled, the library is older than an object or its tag is not this flag set's, the link through exports.map and the tag."""
    if not force and not _needs(sources, headers, out, flags):
        return out
    hipcc = os.environ.get("HIPCC", "hipcc")
    os.makedirs(OBJ_DIR, exist_ok=True)
    plan = _plan(sources, headers, flags)
    jobs = [[hipcc, *flags, "-x", "hip", "-c", deps[0], "-o", o] for o, deps in plan if force or _stale(o, deps)]

    def run(cmd):
        if verbose:
            print(" ".join(cmd), flush=True)
        subprocess.run(cmd, check=True, cwd=HERE)
    with concurrent.futures.ThreadPoolExecutor(max_workers=min(4, max(1, len(jobs)))) as ex:
        list(ex.map(run, jobs))
    tag = out + ".tag"
    if os.path.exists(tag):
        os.remove(tag)          # no tag while the library is being replaced
    # exports.map: only dsdtm_* leaves a library (release: exactly the header's symbols; diag: + dsdtm_debug_*)
    run([hipcc, "--offload-arch=gfx950", "-fPIC", "-shared", "-fno-gpu-rdc", "-Wl,--version-script=" + os.path.join(HERE, "exports.map"),
         *[o for o, _ in plan], "-o", out])
    with open(tag, "w") as f:
        f.write(_tag(flags) + "\n")
    return out


def needs_build(extra=(), diag=False):
    return _needs(_sources(diag), HEADERS, out_path(diag), _flags(list(extra), diag))


def build(force=False, verbose=True, extra=(), diag=False):
    return _make(_sources(diag), HEADERS, out_path(diag), _flags(list(extra), diag), force, verbose)


def _addon(name):
    return ADDONS[name] if name in ADDONS else MORE_ADDONS[name]


def addon_needs_build(name):
    sources, headers, out = _addon(name)
    return _needs(sources, headers, out, _flags([]))


def build_addon(name, force=False, verbose=True):
    """An add-on library of the tables above, with the release flags."""
    sources, headers, out = _addon(name)
    return _make(sources, headers, out, _flags([]), force, verbose)


def build_keyframe(force=False, verbose=True):
    return build_addon("keyframe", force, verbose)


def build_motion(force=False, verbose=True):
    return build_addon("motion", force, verbose)


def build_all(force=False, verbose=True):
    """The release library and the diagnostic one (what __graft_entry__.build() and the test session build), and every add-on."""
    for name in (*ADDONS, *MORE_ADDONS):
        build_addon(name, force, verbose)
    return build(force, verbose), build(force, verbose, diag=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--force", action="store_true")
    ap.add_argument("--diag", action="store_true", help="build libdsdtm_amd_diag.so (debug entries, environment switches, superseded kernels)")
    ap.add_argument("--all", action="store_true", help="build both libraries and every add-on")
    ap.add_argument("--define", action="append", default=[], help="extra -D for experiments")
    ap.add_argument("--flag", action="append", default=[], help="extra raw compiler flag for experiments, e.g. --flag=-mllvm --flag=-amdgpu-sched-strategy=max-ilp")
    a = ap.parse_args()
    extra = ["-D" + d for d in a.define] + list(a.flag)
    if a.all or not a.diag:
        print(build(a.force, extra=extra))
    if a.all or a.diag:
        print(build(a.force, extra=extra, diag=True))
    if a.all:
        for name in (*ADDONS, *MORE_ADDONS):
            print(build_addon(name, a.force))
