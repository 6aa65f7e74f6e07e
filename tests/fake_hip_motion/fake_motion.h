// tests/fake_hip_motion/fake_motion.h — control interface of the faked motion.hip launches (test infrastructure only).
#pragma once
void fake_motion_fail(long nth);       // the n-th launch (step or feature lookup) from now fails (0: none)
long fake_motion_step_launches();      // step launches that ran
long fake_motion_feature_launches();   // feature-lookup launches that ran
