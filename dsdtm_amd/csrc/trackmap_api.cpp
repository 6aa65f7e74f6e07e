// trackmap_api.cpp — libdsdtm_amd_trackmap.so's host side: the one implementation of the resident track map (trackmap_api_body.h) under
// the names of include/dsdtm_amd_trackmap.h.
#define TM_API(name) dsdtm_trackmap_##name
#define TM_CTX dsdtm_trackmap_ctx
#define TM_LIB "dsdtm_amd_trackmap"
#include "trackmap_api_body.h"
