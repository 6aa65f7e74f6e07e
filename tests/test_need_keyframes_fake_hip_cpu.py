"""dsdtm_need_keyframes without a GPU: the host side of the add-on library (dsdtm_amd/csrc/keyframe_api.cpp) — the context,
the argument checks, the packing of n trackers into one blob, the one upload / one launch / one read-back, every failure path — runs against the unmodified fake HIP runtime of
tests/fake_hip as a stand-alone program (its own main) under AddressSanitizer + UndefinedBehaviorSanitizer (+ LeakSanitizer).
Scenarios: tests/fake_hip_keyframe/driver.cpp; the keyframe.hip launch is faked in tests/fake_hip_keyframe/fake_keyframe.cpp.
Nothing is loaded into Python and nothing is preloaded."""
import os

from tests import fake_hip_build as fhb

HERE = os.path.join(fhb.ROOT, "tests", "fake_hip_keyframe")


def test_need_keyframes_host_side_under_address_and_ub_sanitizers(tmp_path):
    exe = fhb.build_driver(tmp_path, "asan", [os.path.join(HERE, "driver.cpp"), os.path.join(HERE, "fake_keyframe.cpp")], ["keyframe_api.cpp"],
                           include_dirs=[HERE])
    r, lines = fhb.run_driver(exe, "asan")
    assert lines == ["ok keyframe_failures", "ok keyframe_limits", "ok rejected_in_the_middle", "ok create_failures"], lines
