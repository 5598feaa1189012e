// decode_shared.hip -- the shared-prefix step of the paged one-row decode (dta_attn_decode_paged_shared*).
// The group pass and the one-row pass that follows it are decode.hip's split kernel instantiated
// with MODE 1 and 2 (see "shared-prefix plan" there); this unit holds those instantiations, the
// one-row combine, their launchers and launch_decode_shared*.  A unit of its own so that the
// build compiles it next to decode.hip instead of after it.
#define DTA_DECODE_GROUP_TU
#include "decode.hip"
