/* K32's part of the C-ABI (include/wga_hip.h): the two entries as a binding in another language calls them, the struct they
 * take, and the ABI version an addition leaves alone. */
#include <stddef.h>

#include "wga_hip.h"

_Static_assert(WGA_ABI_VERSION == 3, "K32 is an addition");
_Static_assert(sizeof(wga_maf_frame_head) == 88, "wga_maf_frame_head");
_Static_assert(offsetof(wga_maf_frame_head, score) == 0 && offsetof(wga_maf_frame_head, t) == 8 &&
                   offsetof(wga_maf_frame_head, q) == 32,
               "wga_maf_frame_head: the numbers");
_Static_assert(offsetof(wga_maf_frame_head, tname_off) == 56 && offsetof(wga_maf_frame_head, qname_off) == 64 &&
                   offsetof(wga_maf_frame_head, tname_len) == 72 && offsetof(wga_maf_frame_head, qname_len) == 76,
               "wga_maf_frame_head: the spans");
_Static_assert(offsetof(wga_maf_frame_head, t_neg) == 80 && offsetof(wga_maf_frame_head, q_neg) == 81 &&
                   offsetof(wga_maf_frame_head, pad) == 82,
               "wga_maf_frame_head: the strands");
_Static_assert(sizeof(wga_cigar_counts) == 88, "wga_cigar_counts");
_Static_assert(sizeof(wga_rec_diag) == 24 && offsetof(wga_rec_diag, bad_op_idx) == 0 && offsetof(wga_rec_diag, panic_op_idx) == 8 &&
                   offsetof(wga_rec_diag, bad_base_pos) == 16,
               "wga_rec_diag");

/* the declarations have these types */
static uint64_t (*const work_bytes)(uint64_t) = wga_paf2maf_frame_work_bytes;
static int (*const frame)(wga_ctx*, uint32_t, const uint8_t*, uint64_t, const wga_maf_frame_head*, const wga_cigar_counts*,
                          const uint64_t*, const uint64_t*, const wga_rec_diag*, void*, uint64_t*, uint64_t*, uint64_t*, uint64_t*,
                          uint32_t*, uint64_t*, uint8_t*) = wga_paf2maf_frame;

const void* abi_layout_maf_frame_refs(void) { return work_bytes && frame ? (const void*)0 : (const void*)1; }
