// control of the fakes of framediff.hip's launch functions (fake_framediff.cpp). Test infrastructure only.
#pragma once
void fake_framediff_fail(long nth);      // the n-th launch from now returns hipErrorUnknown (once); 0: none
long fake_framediff_launches();
