/* The layout of K25's struct (include/wga_hip.h): the numbers a binding in another language has to reproduce. */
#include <stddef.h>

#include "wga_hip.h"

_Static_assert(sizeof(wga_chain_filter_params) == 16, "wga_chain_filter_params");
_Static_assert(offsetof(wga_chain_filter_params, min_block_size) == 0, "min_block_size");
_Static_assert(offsetof(wga_chain_filter_params, min_query_size) == 8, "min_query_size");

_Static_assert(WGA_ABI_VERSION == 3, "K25 is an addition: the ABI version stays");
