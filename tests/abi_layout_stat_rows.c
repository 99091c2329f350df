/* K33's part of the C-ABI (include/wga_hip.h): the three entries as a binding in another language calls them, the struct they
 * take, and the ABI version an addition leaves alone. */
#include <stddef.h>

#include "wga_hip.h"

_Static_assert(WGA_ABI_VERSION == 3, "K33 is an addition");
/* four numbers, two 64-bit offsets, two 32-bit lengths: 56 bytes, no padding */
_Static_assert(sizeof(wga_stat_row_head) == 56, "wga_stat_row_head");
_Static_assert(offsetof(wga_stat_row_head, ref_size) == 0 && offsetof(wga_stat_row_head, ref_start) == 8 &&
                   offsetof(wga_stat_row_head, query_size) == 16 && offsetof(wga_stat_row_head, query_start) == 24,
               "wga_stat_row_head: the numbers");
_Static_assert(offsetof(wga_stat_row_head, rname_off) == 32 && offsetof(wga_stat_row_head, qname_off) == 40 &&
                   offsetof(wga_stat_row_head, rname_len) == 48 && offsetof(wga_stat_row_head, qname_len) == 52,
               "wga_stat_row_head: the spans");
_Static_assert(sizeof(wga_cigar_counts) == 88, "wga_cigar_counts");

/* the declarations have these types */
static uint64_t (*const work_bytes)(uint64_t) = wga_stat_rows_work_bytes;
static int (*const rows)(wga_ctx*, uint32_t, const uint8_t*, uint64_t, const wga_stat_row_head*, const wga_cigar_counts*, void*,
                         uint64_t*, uint64_t*, uint8_t*) = wga_stat_rows;
static int (*const f32_text)(wga_ctx*, uint64_t, const uint32_t*, uint8_t*, uint8_t*) = wga_f32_text;

const void* abi_layout_stat_rows_refs(void) { return work_bytes && rows && f32_text ? (const void*)0 : (const void*)1; }
