"""The HOST side of the C ABI under sanitizers, without a GPU (round-5 verdict, item 4).

dsdtm_amd/csrc/api.cpp and api_*.cpp — stream rings and pair counters, recover slots, the team ring's tag epoch, the sharded / streamed
entries, frames and their buffer pool, the staging blocks every single-call entry and dsdtm_track_frame pack — is compiled with
g++ against a FAKE HIP runtime (tests/fake_hip/: "device" memory in the host heap; every asynchronous operation queued and run
only when something waits for it; fake kernel launchers that touch every buffer a launch names, check the invariants the real
kernels rely on and raise their timeout word on request; any HIP call can be told to fail) and driven through the scenarios of
tests/fake_hip/driver.cpp under AddressSanitizer + UndefinedBehaviorSanitizer (+ LeakSanitizer), and under ThreadSanitizer for
two contexts on two threads. Each of the five lifetime / staleness defects the round-4 advisor found by reading fails one of
these scenarios when its fix is reverted (shown when the job was added: a_no_forget -> heap-use-after-free in
sharded_error_midway; re-run on the context's stream -> recover_slots_past_64; no sticky flag -> evicted_timeout_is_reported;
no second download -> sharded_refetches_after_rerun; no re-zeroing at the epoch wrap -> team_epoch_wrap_hazard_is_real)."""
import os

import pytest

from tests import fake_hip_build as fhb

HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "fake_hip")
SCENARIOS = ["ring_table_past_16_streams", "evicted_timeout_is_reported", "recover_slots_past_64", "team_epoch_wrap_is_cleared",
             "team_epoch_wrap_hazard_is_real", "sharded_refetches_after_rerun", "sharded_error_midway", "streamed_entry", "frame_lifetime",
             "single_call_entries", "device_batch_entries", "refused_levels", "host_batch_one_context", "track_frame_packing", "track_frame_failures", "track_frame_camera_mismatch",
             "two_contexts_two_threads"]


@pytest.fixture(scope="module")
def drivers(tmp_path_factory):
    out = tmp_path_factory.mktemp("fake_hip")
    return [fhb.build_driver(out, san, [os.path.join(HERE, "driver.cpp")], fhb.API_SOURCES, defines=["DSDTM_DIAG=1"]) for san in ("asan", "tsan")]


def test_host_bookkeeping_under_address_and_ub_sanitizers(drivers):
    r, lines = fhb.run_driver(drivers[0], "asan")
    assert lines == ["ok " + s for s in SCENARIOS], lines


def test_two_contexts_on_two_threads_under_thread_sanitizer(drivers):
    r, lines = fhb.run_driver(drivers[1], "tsan",
                              ["two_contexts_two_threads", "ring_table_past_16_streams", "recover_slots_past_64", "sharded_refetches_after_rerun", "streamed_entry"])
    assert len(lines) == 5 and all(l.startswith("ok ") for l in lines), lines
