"""The device-resident track map and dsdtm_trackmap_local without a GPU: the host side of the add-on library
(dsdtm_amd/csrc/trackmap_api.cpp) — the context, the map's six arrays and their growth, the staging ring of the updates, the argument
checks, the packing of n descs, the one upload / one read-back, every failure path — runs against the unmodified fake HIP runtime
of tests/fake_hip as a stand-alone program (its own main) under AddressSanitizer + UndefinedBehaviorSanitizer (+ LeakSanitizer).
Scenarios: tests/fake_hip_trackmap/driver.cpp; the trackmap.hip launches are faked in tests/fake_hip_trackmap/fake_trackmap.cpp, where
the flatten answers with flatten_local_map_host on what it finds in device memory, and the selection's launches are the fakes of
tests/fake_hip_localmap/fake_localmap.cpp (select_local_map_host). Nothing is loaded into Python and nothing is preloaded."""
import os

from tests import fake_hip_build as fhb

HERE = os.path.join(fhb.ROOT, "tests", "fake_hip_trackmap")
LOCALMAP = os.path.join(fhb.ROOT, "tests", "fake_hip_localmap")


def test_track_map_host_side_under_address_and_ub_sanitizers(tmp_path):
    exe = fhb.build_driver(tmp_path, "asan", [os.path.join(HERE, "driver.cpp"), os.path.join(HERE, "fake_trackmap.cpp"), os.path.join(LOCALMAP, "fake_localmap.cpp")],
                           ["trackmap_api.cpp"], include_dirs=[HERE, LOCALMAP])
    r, lines = fhb.run_driver(exe, "asan")
    assert lines == ["ok updates_and_growth", "ok found_write_refusals", "ok validation", "ok hip_failures", "ok limits", "ok create_failures"], (lines, r.stderr[-3000:])
