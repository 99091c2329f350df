/* K35's part of the C-ABI (include/wga_hip.h): the two entries as a binding in another language calls them, the struct they
 * write, the status of a refused table, and the ABI version an addition leaves alone. */
#include <stddef.h>

#include "wga_hip.h"

_Static_assert(WGA_ABI_VERSION == 3, "K35 is an addition");
_Static_assert(WGA_E_FALLBACK == -6 && WGA_E_TOO_SMALL == -5, "the status of a table with a WGA_MAF_FALLBACK line");
/* five 64-bit numbers, two 32-bit ones: 48 bytes, no padding */
_Static_assert(sizeof(wga_maf_index_name) == 48, "wga_maf_index_name");
_Static_assert(offsetof(wga_maf_index_name, name_off) == 0 && offsetof(wga_maf_index_name, size) == 8 &&
                   offsetof(wga_maf_index_name, first_line) == 16 && offsetof(wga_maf_index_name, n_ivls) == 24 &&
                   offsetof(wga_maf_index_name, text_off) == 32 && offsetof(wga_maf_index_name, name_len) == 40 &&
                   offsetof(wga_maf_index_name, isref) == 44,
               "wga_maf_index_name: the fields");
_Static_assert(sizeof(wga_maf_line) == 56, "wga_maf_line");

/* the declarations have these types */
static uint64_t (*const work_bytes)(uint64_t) = wga_maf_index_work_bytes;
static int (*const maf_index)(wga_ctx*, const uint8_t*, uint64_t, const wga_maf_line*, uint64_t, uint32_t, uint64_t, uint64_t, void*,
                          uint64_t*, uint64_t*, uint64_t*, uint64_t*, uint64_t*, uint64_t*, uint64_t*, wga_maf_index_name*,
                          uint8_t*) = wga_maf_index;

const void* abi_layout_maf_index_refs(void) { return work_bytes && maf_index ? (const void*)0 : (const void*)1; }
