// The fp16 instances of include/simaps_spec_store.h (simaps_spec_store.inc), a translation unit of their own.
#define SIMAPS_STORE_DTYPE 2
#include "simaps_spec_store.inc"
