// tests/fake_hip_keyframe/fake_keyframe.h — control interface of the faked keyframe.hip launch (test infrastructure only).
#pragma once
void fake_keyframe_fail(long nth);     // the n-th need_keyframes_launch from now fails (0: none)
long fake_keyframe_launches();         // launches that ran
