// The bf16 kernels of include/simaps_store.h (simaps_store.inc), a translation unit of their own.
#define SIMAPS_STORE_DTYPE 1
#include "simaps_store.inc"
