"""libdsdtm_amd_mapping.so's host side without a GPU: dsdtm_amd/csrc/mapping_api.cpp (over trackmap_api_body.h) — the checks and the
packing of dsdtm_mapping_covisibility, _ba_window and _ba_commit, the event that orders the commit behind the solver's stream, every
refusal, every failing HIP call and launch, the growth of the staging blocks, the memory limit — runs against the unmodified fake HIP
runtime of tests/fake_hip as a stand-alone program (its own main) under AddressSanitizer + UndefinedBehaviorSanitizer (+ LeakSanitizer).
Scenarios: tests/fake_hip_mapping/driver.cpp; the mapping.hip launches are faked in tests/fake_hip_mapping/fake_mapping.cpp by the host
functions of dsdtm_amd/host/dsdtm_mapping_host.hpp, the map's own launches are the fakes of tests/fake_hip_trackmap and
tests/fake_hip_localmap. Nothing is loaded into Python and nothing is preloaded."""
import os

from tests import fake_hip_build as fhb

HERE = os.path.join(fhb.ROOT, "tests", "fake_hip_mapping")
TRACKMAP = os.path.join(fhb.ROOT, "tests", "fake_hip_trackmap")
LOCALMAP = os.path.join(fhb.ROOT, "tests", "fake_hip_localmap")


def test_mapping_host_side_under_address_and_ub_sanitizers(tmp_path):
    exe = fhb.build_driver(tmp_path, "asan", [os.path.join(HERE, "driver.cpp"), os.path.join(HERE, "fake_mapping.cpp"), os.path.join(TRACKMAP, "fake_trackmap.cpp"),
                                              os.path.join(LOCALMAP, "fake_localmap.cpp")], ["mapping_api.cpp"], include_dirs=[HERE, TRACKMAP, LOCALMAP])
    r, lines = fhb.run_driver(exe, "asan")
    assert lines == ["ok windows_and_growth", "ok validation", "ok hip_failures", "ok limits", "ok create_failures"], (lines, r.stderr[-3000:])
