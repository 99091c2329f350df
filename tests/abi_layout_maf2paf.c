/* The layout of K28's struct (include/wga_hip.h): the numbers a binding in another language has to reproduce. */
#include <stddef.h>

#include "wga_hip.h"

_Static_assert(sizeof(wga_maf2paf_head) == 80, "wga_maf2paf_head");
_Static_assert(offsetof(wga_maf2paf_head, q) == 0, "q");
_Static_assert(offsetof(wga_maf2paf_head, t) == 24, "t");
_Static_assert(offsetof(wga_maf2paf_head, qname_off) == 48, "qname_off");
_Static_assert(offsetof(wga_maf2paf_head, tname_off) == 56, "tname_off");
_Static_assert(offsetof(wga_maf2paf_head, qname_len) == 64, "qname_len");
_Static_assert(offsetof(wga_maf2paf_head, tname_len) == 68, "tname_len");
_Static_assert(offsetof(wga_maf2paf_head, strand_neg) == 72, "strand_neg");
_Static_assert(offsetof(wga_maf2paf_head, pad) == 73, "pad");

_Static_assert(WGA_ABI_VERSION == 3, "K28 is an addition: the ABI version stays");
