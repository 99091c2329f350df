/* K36's part of the C-ABI (include/wga_hip.h): the three entries as a binding in another language calls them, the struct they
 * fill, and the ABI version an addition leaves alone. */
#include <stddef.h>

#include "wga_hip.h"

_Static_assert(WGA_ABI_VERSION == 3, "K36 is an addition");
/* four numbers, the eleven counters, the f32's bits and a pad: 128 bytes, no padding */
_Static_assert(sizeof(wga_stat_pair) == 128, "wga_stat_pair");
_Static_assert(offsetof(wga_stat_pair, first_rec) == 0 && offsetof(wga_stat_pair, n_recs) == 8 &&
                   offsetof(wga_stat_pair, ref_start) == 16 && offsetof(wga_stat_pair, query_start) == 24,
               "wga_stat_pair: the numbers");
_Static_assert(offsetof(wga_stat_pair, sum) == 32 && sizeof(((wga_stat_pair*)0)->sum) == 88 && sizeof(wga_cigar_counts) == 88,
               "wga_stat_pair: the sums");
_Static_assert(offsetof(wga_stat_pair, inv_size_bits) == 120 && offsetof(wga_stat_pair, pad) == 124, "wga_stat_pair: the f32");
_Static_assert(sizeof(wga_stat_row_head) == 56, "wga_stat_row_head");

/* the declarations have these types */
static uint64_t (*const work_bytes)(uint64_t) = wga_stat_pairs_work_bytes;
static int (*const pairs)(wga_ctx*, uint32_t, const uint8_t*, uint64_t, const wga_stat_row_head*, const wga_cigar_counts*, void*,
                          uint64_t*, uint32_t*, const uint32_t*, wga_stat_pair*, uint64_t) = wga_stat_pairs;
static int (*const rows)(wga_ctx*, uint32_t, const uint8_t*, uint64_t, const wga_stat_row_head*, const wga_cigar_counts*,
                         const uint32_t*, void*, uint64_t*, uint64_t*, uint8_t*) = wga_stat_pair_rows;

const void* abi_layout_stat_pairs_refs(void) { return work_bytes && pairs && rows ? (const void*)0 : (const void*)1; }
