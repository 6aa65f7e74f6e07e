// mapping_api.cpp — the C ABI of include/dsdtm_amd_mapping.h (libdsdtm_amd_mapping.so). The resident map and its entries are the ONE
// implementation of trackmap_api_body.h, compiled here under the dsdtm_mapping_* names; behind it the three entries of the mapping
// thread, the ONE implementation of mapping_api_body.h under the same names. There is no CPU compute path here (the host evaluation is
// host/dsdtm_mapping_host.hpp, which needs no library).
#define TM_API(name) dsdtm_mapping_##name
#define TM_CTX dsdtm_mapping_ctx
#define TM_LIB "dsdtm_amd_mapping"
#define MP_API(name) dsdtm_mapping_##name
#include "trackmap_api_body.h"
#include "mapping_api_body.h"
