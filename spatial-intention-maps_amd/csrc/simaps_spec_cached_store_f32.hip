// The float32 cached instance of include/simaps_state_cache_store.h (simaps_spec_cached_store.inc), a translation unit of its own.
#define SIMAPS_STORE_DTYPE 0
#include "simaps_spec_cached_store.inc"
