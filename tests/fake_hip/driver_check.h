// tests/fake_hip/driver_check.h — what every driver over the fake HIP runtime shares: the CHECK of a scenario (a `bool` function:
// the first condition that does not hold is printed and fails it) and the 0xA5 prefill of outputs a refused call must not touch.
// Test infrastructure only.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstring>

#define CHECK(cond)                                                                                  \
    do {                                                                                             \
        if (!(cond)) { std::fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); return false; } \
    } while (0)

inline void fill_a5(void* p, size_t bytes) { if (bytes) std::memset(p, 0xA5, bytes); }
inline bool all_a5(const void* p, size_t bytes) {
    for (size_t i = 0; i < bytes; ++i) if (((const uint8_t*)p)[i] != 0xA5) return false;
    return true;
}
