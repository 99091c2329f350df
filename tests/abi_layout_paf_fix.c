/* The layout of K29's struct (include/wga_hip.h): the numbers a binding in another language has to reproduce. */
#include <stddef.h>

#include "wga_hip.h"

_Static_assert(sizeof(wga_paf_fix_sizes) == 48, "wga_paf_fix_sizes");
_Static_assert(offsetof(wga_paf_fix_sizes, rows_bytes) == 0, "rows_bytes");
_Static_assert(offsetof(wga_paf_fix_sizes, qlist_bytes) == 8, "qlist_bytes");
_Static_assert(offsetof(wga_paf_fix_sizes, tlist_bytes) == 16, "tlist_bytes");
_Static_assert(offsetof(wga_paf_fix_sizes, n_records) == 24, "n_records");
_Static_assert(offsetof(wga_paf_fix_sizes, n_q_bad) == 32, "n_q_bad");
_Static_assert(offsetof(wga_paf_fix_sizes, n_t_bad) == 40, "n_t_bad");

_Static_assert(WGA_PAF_FIX_TILE_BYTES == 8192, "the fill's tile");
