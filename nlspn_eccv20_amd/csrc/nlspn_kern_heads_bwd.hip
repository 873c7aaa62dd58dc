// Device code of the head epilogue's backward (nlspn_heads_bwd.h), its own translation unit.
// Launched from nlspn_seam.hip.
#define NLSPN_HEADS_BWD_DEFINE
#include "nlspn_heads_bwd.h"
