// Device code of the resident propagation kernel (nlspn_resident.h) for the geometries
// beyond 3x3: 1x17 and 5x5 (nlspn_resident.h NLSPN_RES_BUILDS_WIDE).  Its own translation
// unit, so it compiles in parallel with the 3x3 builds (nlspn_kern_resident.hip); launched
// from nlspn_prop_fwd.hip.
#include "nlspn_resident.h"

namespace nlspn {
NLSPN_RES_BUILDS_WIDE(NLSPN_RES_INST)
NLSPN_RES_NOCOPY_WIDE(NLSPN_RES_INST_NOCOPY)
}  // namespace nlspn
