/*
 * wga_k26_dotplot_csv.h — K26: the base-level CSV rows of `dotplot --out-format csv` (tools/dotplot.rs:208-262 over the segments
 * of emit_baseplotdatas, cigar.rs:815-914).
 * One header per kernel family; wga_capi.cpp includes them in dependency order (a header may use helpers of the ones in front of it).
 */
#ifndef WGA_K26_DOTPLOT_CSV_H
#define WGA_K26_DOTPLOT_CSV_H

#include "wga_k9_bed.h"      /* dec_digits, dec_write, lds_text_flush */
#include "wga_k12_dotplot.h" /* WGA_SEG_WORDS: the segments as K12 leaves them */

/* ============================================================================================ */
/* K26: dotplot csv row writer                                                                  */
/* ============================================================================================ */
/* Row x of the text is segment x: "<s0>,<s1>,<s2>,<s3>,<M|I|D>" and the TAIL of the segment's record, ",<ref_chro>,<query_chro>\n"
 * as the host's csv quoting made it — opaque bytes here, one tail per record and not per row.  The record of row x is the largest
 * r with seg_off[r] <= x: records without segments (equal neighbours in seg_off) are stepped over wherever they stand.
 *   count  one thread per row: the four numbers' digits + 5 (four commas and the letter) + the tail's length.  A block bisects
 *          twice in seg_off (the records of its first and last row), a thread then only between those two.
 *   scan   the exclusive scan of the row sizes, in place (the shared scan driver over ScanPlain).
 *   fill   256 consecutive rows per block = one contiguous stretch of the text, whatever record borders lie inside it.  The
 *          block's threads write their rows into an LDS image that mirrors the stretch's place inside its 16-byte group, and
 *          the stretch leaves in 16-byte stores (lds_text_flush).  The stage is 256 rows of four 20-digit numbers, the 5 bytes
 *          between them and a tail of 5 bytes (",a,b\n", the shortest two names make): 256 x 90 = 23 040 bytes, 22.5 KiB with
 *          the 32 bytes of alignment slack — seven blocks fit the 160 KiB of a CU, so LDS never holds the kernel below two.  A
 *          block whose stretch is longer (tails of kilobytes) writes its rows directly: correct, slow and rare.
 * A kind above 2 is the caller's error; the letter is then '?' and nothing is indexed by it. */
#define WGA_DOTPLOT_CSV_ROWS 256u
#define WGA_DOTPLOT_CSV_STAGE (WGA_DOTPLOT_CSV_ROWS * 90u)

/* the largest r in [lo, hi) with seg_off[r] <= x (seg_off[lo] <= x): the record of row x.  Always inside [lo, max(hi, lo + 1)),
 * also for offsets that do not ascend */
__device__ __forceinline__ u32 dotplot_row_rec(const u64* __restrict__ seg_off, u32 lo, u32 hi, u64 x) {
  while (lo + 1u < hi) {
    const u32 mid = lo + ((hi - lo) >> 1);
    if (seg_off[mid] <= x) lo = mid; else hi = mid;
  }
  return lo;
}

struct DotRows {
  const u64* segs;
  const u64* seg_off;
  const u8* tails;
  const u64* tail_off;
  u32 n;      /* records */
  u64 n_rows; /* seg_off[n] */
  /* the bytes of row x of record r */
  __device__ __forceinline__ u64 size(u64 x, u32 r) const {
    const u64* s = segs + WGA_SEG_WORDS * x;
    return (u64)(dec_digits(s[0]) + dec_digits(s[1]) + dec_digits(s[2]) + dec_digits(s[3]) + 5u) + (tail_off[r + 1u] - tail_off[r]);
  }
  /* row x of record r at p (LDS or memory) */
  __device__ __forceinline__ void put(u8* p, u64 x, u32 r) const {
    const u64* s = segs + WGA_SEG_WORDS * x;
#pragma unroll
    for (u32 f = 0; f < 4u; f++) {
      const u64 v = s[f];
      const u32 nd = dec_digits(v);
      dec_write(p, v, nd);
      p += nd;
      *p++ = (u8)',';
    }
    const u64 kind = s[4];
    *p++ = kind == 0u ? (u8)'M' : kind == 1u ? (u8)'I' : kind == 2u ? (u8)'D' : (u8)'?';
    const u8* t = tails + tail_off[r];
    const u64 tl = tail_off[r + 1u] - tail_off[r];
    for (u64 k = 0; k < tl; k++) p[k] = t[k];
  }
};

/* s_r[0], s_r[1] = the records of rows x0 and x1 - 1 (two threads bisect; the caller synchronises) */
__device__ __forceinline__ void dotplot_block_recs(const DotRows& R, u64 x0, u64 x1, u32 tid, u32* s_r) {
  if (tid < 2u) s_r[tid] = dotplot_row_rec(R.seg_off, 0u, R.n, tid ? x1 - 1u : x0);
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
  if (x < x1) sizes[x] = R.size(x, dotplot_row_rec(R.seg_off, s_r[0], s_r[1] + 1u, x));
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
  const bool staged = e1 - e0 <= (u64)WGA_DOTPLOT_CSV_STAGE; /* block-uniform */
  u8* const g0 = out + e0;
  const u32 a = (u32)((uintptr_t)g0 & 15u);
  u8* const tbuf = (u8*)s_buf;
  const u64 x = x0 + tid;
  if (x < x1) {
    const u64 at = rsc[x], end = rsc[x + 1u];
    const u32 r = dotplot_row_rec(R.seg_off, s_r[0], s_r[1] + 1u, x);
    if (at >= e0 && end <= e1 && end - at == R.size(x, r)) R.put(staged ? tbuf + a + (u32)(at - e0) : out + at, x, r);
  }
  if (!staged) return;
  __syncthreads();
  lds_text_flush(tbuf, a, (u32)(e1 - e0), g0 - a, tid, 256u);
}

#endif /* WGA_K26_DOTPLOT_CSV_H */
