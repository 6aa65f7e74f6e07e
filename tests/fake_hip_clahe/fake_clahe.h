// Control interface of the fake launches of tests/fake_hip_clahe/fake_clahe.cpp (test infrastructure only).
#pragma once
void fake_clahe_fail(long nth_launch_from_now);      // that launch (tables or interpolation) returns hipErrorUnknown, once; 0: none
long fake_clahe_launches();                          // launches that ran
