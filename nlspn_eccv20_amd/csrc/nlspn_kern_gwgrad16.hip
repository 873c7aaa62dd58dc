// Device code of the split-bf16 weight gradient (nlspn_gwgrad16.h), its own translation unit.
// Launched from nlspn_gconv_host.hip (nlspn_gconv_wgrad_bf16x3).
#include "nlspn_gwgrad16.h"

namespace nlspn {
#define NLSPN_GW16_INST(...) template __global__ void gwgrad16_kernel<__VA_ARGS__>(GwgradArgs);
NLSPN_GW16_CONFIGS(NLSPN_GW16_INST)
}  // namespace nlspn
