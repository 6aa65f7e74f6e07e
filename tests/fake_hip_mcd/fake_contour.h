// tests/fake_hip_mcd/fake_contour.h — control interface of the faked contour.hip launches (test infrastructure only).
#pragma once
void fake_contour_fail(long nth);      // the n-th launch (contour or fill) from now fails (0: none)
long fake_contour_launches();          // contour launches that ran (one per run of masks)
long fake_contour_fill_launches();     // fill launches that ran
