/*
 * wga_k26_dotplot_csv.h — K26: the base-level CSV rows of `dotplot --out-format csv` (tools/dotplot.rs:208-262 over the segments
 * of emit_baseplotdatas, cigar.rs:815-914).
 * One header per kernel family; wga_capi.cpp includes them in dependency order (a header may use helpers of the ones in front of it).
 */
#ifndef WGA_K26_DOTPLOT_CSV_H
#define WGA_K26_DOTPLOT_CSV_H

#include "wga_text_out.h"    /* the sinks, csr_find_in, k_text_items_fill */
#include "wga_k12_dotplot.h" /* WGA_SEG_WORDS: the segments as K12 leaves them */

/* ============================================================================================ */
/* K26: dotplot csv row writer                                                                  */
/* ============================================================================================ */
/* Row x of the text is segment x: "<s0>,<s1>,<s2>,<s3>,<M|I|D>" and the TAIL of the segment's record, ",<ref_chro>,<query_chro>\n"
 * as the host's csv quoting made it — opaque bytes here, one tail per record and not per row.  The record of row x is the largest
 * r with seg_off[r] <= x: records without segments (equal neighbours in seg_off) are stepped over wherever they stand.
 *   count  one thread per row: the row's emitter into a TextCount (the four numbers' digits + 5 for the four commas and the
 *          letter + the tail's length).  A block bisects twice in seg_off (the records of its first and last row, csr_find_in), a
 *          thread then only between those two.
 *   scan   the exclusive scan of the row sizes, in place (the shared scan driver over ScanPlain).
 *   fill   k_text_items_fill<DotRows> (wga_text_out.h): 256 consecutive rows per block, staged and flushed as that file
 *          describes, with the size check on: a row whose size is not the scan's (arrays that are not the count call's) is not
 *          written.  The stage is 256 rows of four 20-digit numbers, the 5 bytes between them and a tail of 5 bytes (",a,b\n", the
 *          shortest two names make): 256 x 90 = 23 040 bytes, 22.5 KiB with the 32 bytes of alignment slack — seven blocks fit
 *          the 160 KiB of a CU, so LDS never holds the kernel below two.  A block whose stretch is longer (tails of kilobytes)
 *          writes its rows directly.
 * A kind above 2 is the caller's error; the letter is then '?' and nothing is indexed by it. */
#define WGA_DOTPLOT_CSV_STAGE (WGA_TEXT_ITEMS * 90u)

/* the arrays, and with them the format of the rows (wga_text_out.h) */
struct DotRows {
  static constexpr u32 kStage = WGA_DOTPLOT_CSV_STAGE;
  static constexpr bool kCheckSize = true;
  const u64* segs;
  const u64* seg_off;
  const u8* tails;
  const u64* tail_off;
  u32 n_rec;  /* records */
  u64 n_rows; /* seg_off[n_rec] */
  __device__ __forceinline__ u32 rec(u64 x, u32 lo, u32 hi) const { return csr_find_in(seg_off, lo, hi, x); }
  /* row x of record r */
  template <typename S>
  __device__ __forceinline__ void emit(S& s, u64 x, u32 r) const {
    const u64* v = segs + WGA_SEG_WORDS * x;
#pragma unroll
    for (u32 f = 0; f < 4u; f++) {
      s.dec(v[f]);
      s.c((u8)',');
    }
    const u64 kind = v[4];
    s.c(kind == 0u ? (u8)'M' : kind == 1u ? (u8)'I' : kind == 2u ? (u8)'D' : (u8)'?');
    const u8* t = tails + tail_off[r];
    u64 tl = tail_off[r + 1u] - tail_off[r];
    for (; tl > 0xFFFFFFFFull; tl -= 0x80000000ull, t += 0x80000000ull) s.str(t, 0x80000000u); /* a tail's length is a u64, a span's a u32 */
    s.str(t, (u32)tl);
  }
  __device__ __forceinline__ u64 size(u64 x, u32 r) const {
    TextCount c;
    emit(c, x, r);
    return c.n;
  }
};

/* sizes[x] = the bytes of row x */
__global__ __launch_bounds__(256) void k_dotplot_csv_count(DotRows R, u64* __restrict__ sizes) {
  __shared__ u32 s_r[2];
  const u32 tid = threadIdx.x;
  const u64 x0 = (u64)blockIdx.x * WGA_TEXT_ITEMS;
  const u64 x1 = x0 + WGA_TEXT_ITEMS < R.n_rows ? x0 + WGA_TEXT_ITEMS : R.n_rows;
  if (tid < 2u) s_r[tid] = R.rec(tid ? x1 - 1u : x0, 0u, R.n_rec); /* the records of the first and the last row */
  __syncthreads();
  const u64 x = x0 + tid;
  if (x < x1) sizes[x] = R.size(x, R.rec(x, s_r[0], s_r[1] + 1u));
}

#endif /* WGA_K26_DOTPLOT_CSV_H */
