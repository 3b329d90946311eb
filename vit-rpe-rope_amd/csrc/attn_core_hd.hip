// Attention core (attn_core.h) at the head dimensions beyond 32 / 64: 24 and 48 on padded tiles (hd 32 / 64 layouts,
// PadMap), 96 and 128 on their own.  The Makefile compiles this file once per head dimension (-DVITPE_CORE_HD=24 ...)
// so that the instantiations build in parallel; without the macro (tools/regs.sh) it instantiates every head dimension
// that VITPE_CORE_HDS marks as having its own translation unit.
#define VITPE_CORE_HD_TU
#include "attn_core.h"
