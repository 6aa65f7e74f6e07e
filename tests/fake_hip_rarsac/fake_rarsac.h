// tests/fake_hip_rarsac/fake_rarsac.h — control interface of the faked rarsac.hip launch (test infrastructure only).
#pragma once
void fake_rarsac_fail(long nth);   // the n-th launch from now fails (0: none)
long fake_rarsac_launches();       // launches that ran
