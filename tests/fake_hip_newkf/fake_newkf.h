// Control interface of the fake launch of dsdtm_amd/csrc/newkf.hip (fake_newkf.cpp). Test infrastructure only.
#pragma once
void fake_newkf_fail(long nth);            // the n-th launch from now returns hipErrorUnknown (once); 0 = none
long fake_newkf_launches();
// the addresses the LAST launch was given for tracker t: what the kernel would read the cells' scores, the depth and the mask from
const void* fake_newkf_seen(int t, int which);      // which: 0 cell_score, 1 depth, 2 dyn_mask, 3 cell_x
