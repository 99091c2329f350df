/*
 * wga_k26_dotplot_csv.h — K26: the base-level CSV rows of `dotplot --out-format csv` (tools/dotplot.rs:208-262 over the segments
 * of emit_baseplotdatas, cigar.rs:815-914).
 * One header per kernel family; wga_capi.cpp includes them in dependency order (a header may use helpers of the ones in front of it).
 */
#ifndef WGA_K26_DOTPLOT_CSV_H
#define WGA_K26_DOTPLOT_CSV_H

#include "wga_text_out.h"    /* the sinks, TextStretch, csr_find_in */
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
 *   fill   256 consecutive rows per block = one contiguous stretch of the text, whatever record borders lie inside it, staged and
 *          flushed as wga_text_out.h describes.  The stage is 256 rows of four 20-digit numbers, the 5 bytes between them and a
 *          tail of 5 bytes (",a,b\n", the shortest two names make): 256 x 90 = 23 040 bytes, 22.5 KiB with the 32 bytes of
 *          alignment slack — seven blocks fit the 160 KiB of a CU, so LDS never holds the kernel below two.  A block whose stretch
 *          is longer (tails of kilobytes) writes its rows directly.
 * A kind above 2 is the caller's error; the letter is then '?' and nothing is indexed by it. */
#define WGA_DOTPLOT_CSV_ROWS 256u
#define WGA_DOTPLOT_CSV_STAGE (WGA_DOTPLOT_CSV_ROWS * 90u)

struct DotRows {
  const u64* segs;
  const u64* seg_off;
  const u8* tails;
  const u64* tail_off;
  u32 n;      /* records */
  u64 n_rows; /* seg_off[n] */
};
/* row x of record r */
template <typename S>
__device__ __forceinline__ void dotplot_row_emit(S& s, const DotRows& R, u64 x, u32 r) {
  const u64* v = R.segs + WGA_SEG_WORDS * x;
#pragma unroll
  for (u32 f = 0; f < 4u; f++) {
    s.dec(v[f]);
    s.c((u8)',');
  }
  const u64 kind = v[4];
  s.c(kind == 0u ? (u8)'M' : kind == 1u ? (u8)'I' : kind == 2u ? (u8)'D' : (u8)'?');
  const u8* t = R.tails + R.tail_off[r];
  u64 tl = R.tail_off[r + 1u] - R.tail_off[r];
  for (; tl > 0xFFFFFFFFull; tl -= 0x80000000ull, t += 0x80000000ull) s.str(t, 0x80000000u); /* a tail's length is a u64, a span's a u32 */
  s.str(t, (u32)tl);
}
__device__ __forceinline__ u64 dotplot_row_size(const DotRows& R, u64 x, u32 r) {
  TextCount c;
  c.n = 0;
  dotplot_row_emit(c, R, x, r);
  return c.n;
}

/* s_r[0], s_r[1] = the records of rows x0 and x1 - 1 (two threads bisect; the caller synchronises) */
__device__ __forceinline__ void dotplot_block_recs(const DotRows& R, u64 x0, u64 x1, u32 tid, u32* s_r) {
  if (tid < 2u) s_r[tid] = csr_find_in(R.seg_off, 0u, R.n, tid ? x1 - 1u : x0);
}

/* sizes[x] = the bytes of row x */
__global__ __launch_bounds__(256) void k_dotplot_csv_count(DotRows R, u64* __restrict__ sizes) {
  __shared__ u32 s_r[2];
  const u32 tid = threadIdx.x;
  const u64 x0 = (u64)blockIdx.x * WGA_DOTPLOT_CSV_ROWS;
  const u64 x1 = x0 + WGA_DOTPLOT_CSV_ROWS < R.n_rows ? x0 + WGA_DOTPLOT_CSV_ROWS : R.n_rows;
  dotplot_block_recs(R, x0, x1, tid, s_r);
  __syncthreads();
  const u64 x = x0 + tid;
  if (x < x1) sizes[x] = dotplot_row_size(R, x, csr_find_in(R.seg_off, s_r[0], s_r[1] + 1u, x));
}

/* rows [256 b, 256 b + 256); rsc = the exclusive scan of the row sizes (rsc[n_rows] = the text's length).  Nothing is written
 * outside out[0, total): a block whose stretch ends behind `total`, and a row whose size is not the scan's (arrays that are not
 * the count call's), write nothing. */
__global__ __launch_bounds__(256) void k_dotplot_csv_fill(DotRows R, const u64* __restrict__ rsc, u64 total, u8* __restrict__ out) {
  __shared__ u32x4_a16 s_buf[(WGA_DOTPLOT_CSV_STAGE + 32u) / 16u];
  __shared__ u32 s_r[2];
  const u32 tid = threadIdx.x;
  const u64 x0 = (u64)blockIdx.x * WGA_DOTPLOT_CSV_ROWS;
  const u64 x1 = x0 + WGA_DOTPLOT_CSV_ROWS < R.n_rows ? x0 + WGA_DOTPLOT_CSV_ROWS : R.n_rows;
  const u64 e0 = rsc[x0], e1 = rsc[x1]; /* bytes in front of the block, and behind it */
  if (e1 <= e0 || e1 > total) return;   /* block-uniform */
  dotplot_block_recs(R, x0, x1, tid, s_r);
  __syncthreads();
  const TextStretch st(s_buf, WGA_DOTPLOT_CSV_STAGE, out + e0, e1 - e0); /* block-uniform */
  const u64 x = x0 + tid;
  if (x < x1) {
    const u64 at = rsc[x], end = rsc[x + 1u];
    const u32 r = csr_find_in(R.seg_off, s_r[0], s_r[1] + 1u, x);
    if (at >= e0 && end <= e1 && end - at == dotplot_row_size(R, x, r)) {
      TextPut w;
      w.p = st.at(at - e0);
      dotplot_row_emit(w, R, x, r);
    }
  }
  st.flush_block(tid);
}

#endif /* WGA_K26_DOTPLOT_CSV_H */
