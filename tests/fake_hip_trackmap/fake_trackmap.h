// tests/fake_hip_trackmap/fake_trackmap.h — control interface of the faked trackmap.hip launches (test infrastructure only).
#pragma once
void fake_trackmap_fail(long nth);      // the n-th launch (apply, points, found or flatten) from now fails (0: none)
long fake_trackmap_flatten_launches();  // flatten launches that ran
long fake_trackmap_update_launches();   // apply + points + found launches that ran
