// Device code of the resident propagation kernel (nlspn_resident.h), compiled as its
// own translation unit so its code-generation flags can differ from the rest of the
// library (see Makefile) and so it rebuilds in parallel with the other units.  The
// host stubs instantiated here are launched from nlspn_prop_fwd.hip.
#include "nlspn_resident.h"

namespace nlspn {
// The 3x3 builds (nlspn_resident.h NLSPN_RES_BUILDS_3X3); the wider geometries' are
// nlspn_kern_resident_wide.hip.
NLSPN_RES_BUILDS_3X3(NLSPN_RES_INST)
// ... and the loop-copy builds without the copy code (NLSPN_RES_NOCOPY_3X3)
NLSPN_RES_NOCOPY_3X3(NLSPN_RES_INST_NOCOPY)
}  // namespace nlspn
