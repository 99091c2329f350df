/* K31's part of the C-ABI (include/wga_hip.h): the entry as a binding in another language calls it, the item it reads, the four
 * kinds, and the ABI version an addition leaves alone. */
#include <stddef.h>

#include "wga_hip.h"

_Static_assert(WGA_ABI_VERSION == 3, "K31 is an addition");
_Static_assert(sizeof(wga_span_item) == 32, "wga_span_item");
_Static_assert(offsetof(wga_span_item, dst) == 0 && offsetof(wga_span_item, len) == 8 && offsetof(wga_span_item, src) == 16 &&
                   offsetof(wga_span_item, kind) == 24 && offsetof(wga_span_item, pad) == 28,
               "wga_span_item");
_Static_assert(WGA_SPAN_FILL == 0u && WGA_SPAN_COPY_POOL == 1u && WGA_SPAN_COPY_TEXT == 2u && WGA_SPAN_HOLE == 3u, "the kinds");
_Static_assert(WGA_PSEUDO_FRAME_TILE % 16u == 0u && WGA_PSEUDO_FRAME_TILE >= 4096u, "whole 16-byte groups per tile");

/* the declaration has this type */
static int (*const frame)(wga_ctx*, uint64_t, const wga_span_item*, const uint8_t*, uint64_t, const uint8_t*, uint64_t, uint8_t*,
                          uint64_t, uint64_t*) = wga_pafpseudo_frame;

const void* abi_layout_pseudo_frame_refs(void) { return frame ? (const void*)0 : (const void*)1; }
