// Attention core (attn_core.h) at the head dimensions beyond 32 / 64: 24 and 48 on padded tiles (hd 32 / 64 layouts,
// PadMap), 96 and 128 on their own.  The Makefile compiles this file once per head dimension (-DVITPE_CORE_HD=24 ...)
// so that the instantiations build in parallel; without the macro (tools/regs.sh) it instantiates all four.
#define VITPE_CORE_HD_TU
#include "attn_core.h"

namespace vitpe {

#define VITPE_CORE_INSTANTIATE_HD(HD)                                                      \
  template int dispatch_core_t<bf16, HD>(bool, int, const AttnArgs&, hipStream_t);         \
  template int dispatch_core_t<float, HD>(bool, int, const AttnArgs&, hipStream_t);        \
  template bool core_supported_t<bf16, HD>(int);                                           \
  template bool core_supported_t<float, HD>(int);

#ifdef VITPE_CORE_HD
VITPE_CORE_INSTANTIATE_HD(VITPE_CORE_HD)
#else
VITPE_CORE_INSTANTIATE_HD(24)
VITPE_CORE_INSTANTIATE_HD(48)
VITPE_CORE_INSTANTIATE_HD(96)
VITPE_CORE_INSTANTIATE_HD(128)
#endif

}  // namespace vitpe
