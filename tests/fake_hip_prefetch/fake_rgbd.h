// tests/fake_hip_prefetch/fake_rgbd.h — control interface of the faked rgbd.hip launches (test infrastructure only).
#pragma once
void fake_rgbd_fail(long depth_nth, long lift_nth);   // the n-th depth_ingest_launch / lift_launch from now fails (0: none)
long fake_rgbd_depth_launches();
float fake_rgbd_last_inv_scale();
