// Device code of the f16-operand GRU-mode convolutions (nlspn_gconv16.h), their own translation
// unit.  Launched from nlspn_gconv_host.hip (nlspn_gconv16); the configurations are
// NLSPN_GC16_CONFIGS.
#include "nlspn_gconv16.h"

namespace nlspn {
#define NLSPN_GC16_INST(id, ...) template __global__ void gconv16_kernel<__VA_ARGS__>(Gconv16Args);
NLSPN_GC16_CONFIGS(NLSPN_GC16_INST)
template __global__ void gsmall16_kernel<16>(Gconv16Args, const float *);
}  // namespace nlspn
