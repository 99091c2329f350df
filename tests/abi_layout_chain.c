/* The layout of the chain reader's head (include/wga_hip.h, wga_chain_split): the size and every offset a binding in another
 * language has to reproduce (INTEGRATION.md section 2 quotes them).  Compiled by tests/test_abi_chain.py; never linked. */
#include <stddef.h>

#include "wga_hip.h"

_Static_assert(sizeof(wga_chain_head) == 96, "wga_chain_head");
_Static_assert(offsetof(wga_chain_head, num) == 0, "wga_chain_head.num");
_Static_assert(offsetof(wga_chain_head, tname_off) == 64, "wga_chain_head.tname_off");
_Static_assert(offsetof(wga_chain_head, qname_off) == 72, "wga_chain_head.qname_off");
_Static_assert(offsetof(wga_chain_head, tname_len) == 80, "wga_chain_head.tname_len");
_Static_assert(offsetof(wga_chain_head, qname_len) == 84, "wga_chain_head.qname_len");
_Static_assert(offsetof(wga_chain_head, tstrand_neg) == 88, "wga_chain_head.tstrand_neg");
_Static_assert(offsetof(wga_chain_head, qstrand_neg) == 89, "wga_chain_head.qstrand_neg");
_Static_assert(offsetof(wga_chain_head, pad) == 90, "wga_chain_head.pad");
_Static_assert(WGA_CHAIN_OK == 0 && WGA_CHAIN_FALLBACK == 1, "chain status");
_Static_assert(WGA_ABI_VERSION == 3, "an addition only");
