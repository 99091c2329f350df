/* The layouts of K24's structs (include/wga_hip.h): the numbers a binding in another language has to reproduce. */
#include <stddef.h>

#include "wga_hip.h"

_Static_assert(sizeof(wga_paf_pair) == 40, "wga_paf_pair");
_Static_assert(offsetof(wga_paf_pair, first_line) == 0, "first_line");
_Static_assert(offsetof(wga_paf_pair, sum) == 8, "sum");
_Static_assert(offsetof(wga_paf_pair, qname_off) == 16, "qname_off");
_Static_assert(offsetof(wga_paf_pair, tname_off) == 24, "tname_off");
_Static_assert(offsetof(wga_paf_pair, qname_len) == 32, "qname_len");
_Static_assert(offsetof(wga_paf_pair, tname_len) == 36, "tname_len");

_Static_assert(sizeof(wga_paf_filter_params) == 32, "wga_paf_filter_params");
_Static_assert(offsetof(wga_paf_filter_params, min_block_size) == 0, "min_block_size");
_Static_assert(offsetof(wga_paf_filter_params, min_query_size) == 8, "min_query_size");
_Static_assert(offsetof(wga_paf_filter_params, d_pair_of_line) == 16, "d_pair_of_line");
_Static_assert(offsetof(wga_paf_filter_params, d_pair_keep) == 24, "d_pair_keep");

_Static_assert(WGA_PAF_FILTER_TILE_BYTES == 8192, "the fill's tile");
