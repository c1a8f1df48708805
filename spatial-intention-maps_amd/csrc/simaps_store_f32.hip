// The float32 kernel of include/simaps_store.h (simaps_store.inc), a translation unit of its own.
#define SIMAPS_STORE_DTYPE 0
#include "simaps_store.inc"
