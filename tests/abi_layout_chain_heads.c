/* K30's part of the C-ABI (include/wga_hip.h): the two entries as a binding in another language calls them, the struct they
 * reuse, and the ABI version an addition leaves alone. */
#include <stddef.h>

#include "wga_hip.h"

_Static_assert(WGA_ABI_VERSION == 3, "K30 is an addition");
_Static_assert(sizeof(wga_maf2paf_head) == 80, "wga_maf2paf_head");
_Static_assert(offsetof(wga_maf2paf_head, qname_off) == 48 && offsetof(wga_maf2paf_head, strand_neg) == 72, "wga_maf2paf_head");
_Static_assert(sizeof(wga_chain_trim_t) == 32, "wga_chain_trim_t");
_Static_assert(sizeof(wga_rec_diag) == 24 && offsetof(wga_rec_diag, bad_op_idx) == 0, "wga_rec_diag");

/* the declarations have these types */
static uint64_t (*const work_bytes)(uint64_t) = wga_chain_heads_work_bytes;
static int (*const heads)(wga_ctx*, uint32_t, const uint8_t*, uint64_t, const wga_maf2paf_head*, const wga_chain_trim_t*,
                          const uint64_t*, const wga_rec_diag*, uint64_t, void*, uint64_t*, uint64_t*, uint32_t*,
                          uint8_t*) = wga_chain_heads;

const void* abi_layout_chain_heads_refs(void) { return work_bytes && heads ? (const void*)0 : (const void*)1; }
