// Control interface of the fake launches of mapping.hip (tests/fake_hip_mapping/fake_mapping.cpp). Test infrastructure only.
#pragma once
void fake_mapping_fail(long nth);      // the nth launch of mapping.hip from now returns hipErrorUnknown (once); 0: none
long fake_mapping_launches();
