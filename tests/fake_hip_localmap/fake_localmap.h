// tests/fake_hip_localmap/fake_localmap.h — control interface of the faked localmap.hip launches (test infrastructure only).
#pragma once
void fake_localmap_fail(long nth);     // the n-th launch (apply or select) from now fails (0: none)
long fake_localmap_select_launches();  // select launches that ran
long fake_localmap_apply_launches();   // apply launches that ran
