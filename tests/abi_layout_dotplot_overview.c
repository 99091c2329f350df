/* K34's part of the C-ABI (include/wga_hip.h): the three entries as a binding in another language calls them, the struct they
 * take, and the ABI version an addition leaves alone. */
#include <stddef.h>

#include "wga_hip.h"

_Static_assert(WGA_ABI_VERSION == 3, "K34 is an addition");
/* four numbers and the divisor, two 64-bit offsets, two 32-bit lengths: 64 bytes, no padding */
_Static_assert(sizeof(wga_dotplot_ov_head) == 64, "wga_dotplot_ov_head");
_Static_assert(offsetof(wga_dotplot_ov_head, ref_start) == 0 && offsetof(wga_dotplot_ov_head, ref_end) == 8 &&
                   offsetof(wga_dotplot_ov_head, q_first) == 16 && offsetof(wga_dotplot_ov_head, q_second) == 24 &&
                   offsetof(wga_dotplot_ov_head, align_size) == 32,
               "wga_dotplot_ov_head: the numbers");
_Static_assert(offsetof(wga_dotplot_ov_head, rname_off) == 40 && offsetof(wga_dotplot_ov_head, qname_off) == 48 &&
                   offsetof(wga_dotplot_ov_head, rname_len) == 56 && offsetof(wga_dotplot_ov_head, qname_len) == 60,
               "wga_dotplot_ov_head: the spans");
_Static_assert(sizeof(wga_cigar_counts) == 88 && offsetof(wga_cigar_counts, match) == 0, "wga_cigar_counts");

/* the declarations have these types */
static uint64_t (*const work_bytes)(uint64_t) = wga_dotplot_overview_work_bytes;
static int (*const rows)(wga_ctx*, uint32_t, const uint8_t*, uint64_t, const wga_dotplot_ov_head*, const wga_cigar_counts*, int, void*,
                         uint64_t*, uint64_t*, uint8_t*) = wga_dotplot_overview;
static int (*const f64_text)(wga_ctx*, uint64_t, const uint64_t*, uint8_t*, uint8_t*) = wga_f64_text;

const void* abi_layout_dotplot_overview_refs(void) { return work_bytes && rows && f64_text ? (const void*)0 : (const void*)1; }
