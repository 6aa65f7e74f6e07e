// Control interface of the fake launch of aftertrack.hip (tests/fake_hip_slam/fake_slam.cpp). Test infrastructure only.
#pragma once
void fake_slam_fail(long nth);         // the nth launch of aftertrack.hip from now returns hipErrorUnknown (once); 0: none
long fake_slam_launches();
