// Device code of the head-epilogue convolution kernel (nlspn_heads.h), its own
// translation unit (it rebuilds in parallel with the other units).  Launched from
// nlspn_seam.hip.
#include "nlspn_heads.h"

namespace nlspn {
NLSPN_HD_BUILDS(NLSPN_HD_INST)
}  // namespace nlspn
