// The bf16 instantiation of get_state_kernel (simaps_state16.inc), a translation unit of its own.
#define SIMAPS_STATE16 1
#include "simaps_state16.inc"
