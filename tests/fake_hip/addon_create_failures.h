// tests/fake_hip/addon_create_failures.h — the scenario `create_failures` of every add-on library's driver: the failure paths of
// <prefix>_create, which dsdtm_amd/csrc/addon_host.h owns for all of them. Include behind the add-on's public header (DSDTM_* status
// codes). `lib_name`: the library as its messages call it. Test infrastructure only.
#pragma once
#include <cstdint>
#include <cstring>

#include "driver_check.h"
#include "fake_hip.h"

template <class Ctx>
static bool addon_create_failures(const char* lib_name, int (*create)(int, Ctx**), void (*destroy)(Ctx*), const char* (*last_error)(const Ctx*)) {
    Ctx* const stale = (Ctx*)(uintptr_t)1;
    Ctx* ctx = stale;
    CHECK(create(0, nullptr) == DSDTM_ERR_INVALID);
    // no device to be seen: the message names the library and that nothing else computes
    fake_hip_fail("hipGetDeviceCount", 1);
    CHECK(create(0, &ctx) == DSDTM_ERR_NO_DEVICE && ctx == nullptr);
    fake_hip_fail("hipGetDeviceCount", 0);
    CHECK(strstr(last_error(nullptr), lib_name) && strstr(last_error(nullptr), "no CPU fallback"));
    // a device that is not there (the fake reports two)
    for (int device : {-1, 2}) {
        ctx = stale;
        CHECK(create(device, &ctx) == DSDTM_ERR_NO_DEVICE && ctx == nullptr && strstr(last_error(nullptr), "out of range"));
    }
    // no stream: the context that was allocated is freed (LeakSanitizer would report it)
    ctx = stale;
    fake_hip_fail("hipStreamCreateWithFlags", 1);
    CHECK(create(0, &ctx) == DSDTM_ERR_HIP && ctx == nullptr);
    fake_hip_fail("hipStreamCreateWithFlags", 0);
    CHECK(strlen(last_error(nullptr)) > 0);
    // and none of this stands in the way of the next create
    CHECK(create(1, &ctx) == DSDTM_OK && ctx != nullptr);
    destroy(ctx);
    CHECK(fake_hip_live_allocations() == 0 && fake_hip_pending() == 0);
    CHECK(fake_hip_errors().empty());
    return true;
}
