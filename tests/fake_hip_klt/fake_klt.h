// tests/fake_hip_klt/fake_klt.h — control interface of the faked launches of klt.hip (test infrastructure only).
#pragma once
void fake_klt_fail(long nth);   // the n-th launch from now (ingest, Lucas-Kanade or compaction) fails (0: none)
long fake_klt_launches();       // launches that ran
