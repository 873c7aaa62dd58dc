// Device code of the split-bf16 GRU-mode convolutions (nlspn_gconv_x3.h), their own translation
// unit.  Launched from nlspn_gconv_host.hip (nlspn_gconv_x3); the configurations are
// NLSPN_GCX3_CONFIGS.
#include "nlspn_gconv_x3.h"

namespace nlspn {
#define NLSPN_GCX3_INST(id, ...) template __global__ void gconvx3_kernel<__VA_ARGS__>(GconvX3Args);
NLSPN_GCX3_CONFIGS(NLSPN_GCX3_INST)
template __global__ void gsmallx3_kernel<16>(GconvX3Args, const float *);
}  // namespace nlspn
