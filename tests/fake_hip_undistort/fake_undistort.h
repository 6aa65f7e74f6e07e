// Control interface of the fake launches of tests/fake_hip_undistort/fake_undistort.cpp (test infrastructure only).
#pragma once
void fake_undistort_fail(long nth_launch_from_now);      // that launch (map, frames or points) returns hipErrorUnknown, once; 0: none
long fake_undistort_launches();                          // launches that ran
