// The fp16 instantiation of get_state_kernel (simaps_state16.inc), a translation unit of its own.
#define SIMAPS_STATE16 2
#include "simaps_state16.inc"
