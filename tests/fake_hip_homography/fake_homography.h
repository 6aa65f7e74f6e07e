// tests/fake_hip_homography/fake_homography.h — control interface of the faked homography.hip launch (test infrastructure only).
#pragma once
void fake_homography_fail(long nth);   // the n-th launch from now fails (0: none)
long fake_homography_launches();       // launches that ran
