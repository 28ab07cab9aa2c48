// capi.cpp — the C ABI declared in include/dynfu_amd.h, first unit: the error buffer every unit writes (capi_internal.hpp)
// and the entry points that describe the library.  The seams are in capi_tsdf.cpp, capi_field.cpp, capi_image.cpp and capi_warp.cpp, the
// two solver plans in capi_solver.cpp and capi_solver6.cpp; no arithmetic lives in any of them, the kernels are in the
// .hip files.
#include "capi_internal.hpp"

__thread char dfa::capi::g_err[512] = "";

using namespace dfa::capi;

extern "C" {

const char* dfa_last_error(void) { return g_err; }

const char* dfa_version(void) { return "dynfu_amd 0.1 (gfx950, HIP)"; }

int dfa_abi_version(void) { return DFA_ABI_VERSION; }

size_t dfa_abi_struct_size(int id) {
    switch (id) {
        case DFA_STRUCT_SOLVE_PARAMS: return sizeof(dfa_solve_params);
        case DFA_STRUCT_SOLVE_STATS: return sizeof(dfa_solve_stats);
        case DFA_STRUCT_SOLVE_TIMING: return sizeof(dfa_solve_timing);
        case DFA_STRUCT_SOLVE6_PARAMS: return sizeof(dfa_solve6_params);
        case DFA_STRUCT_SOLVE6_STATS: return sizeof(dfa_solve6_stats);
        case DFA_STRUCT_SOLVE6_TIMING: return sizeof(dfa_solve6_timing);
        case DFA_STRUCT_KNN_FIELD_DESC: return sizeof(dfa_knn_field_desc);
        default: return 0;
    }
}

}  // extern "C"
