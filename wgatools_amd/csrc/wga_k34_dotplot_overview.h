/*
 * wga_k34_dotplot_overview.h — K34: the csv rows of `dotplot -m overview` (rec_dot_data, tools/dotplot.rs:384-423, written by the
 * csv writer of render_output: comma delimiter, QuoteStyle::Necessary, the f64 column through ryu) over the records' match counts.
 * One header per kernel family; wga_capi.cpp includes them in dependency order (a header may use helpers of the ones in front of it).
 */
#ifndef WGA_K34_DOTPLOT_OVERVIEW_H
#define WGA_K34_DOTPLOT_OVERVIEW_H

#include "wga_text_out.h" /* the sinks, ScanItems, k_text_items_fill and the record rows' skeleton */
#include "wga_paf_head.h" /* csv_field_emit, name_span_len */
#include "wga_f64_text.h" /* f64_text_emit: an f64 as ryu prints it */

/* ============================================================================================ */
/* K34: dotplot overview row writer                                                             */
/* ============================================================================================ */
/* Row r of the text is record r, 7 columns:
 *   <ref_start>,<ref_end>,<q_first>,<q_second>,<identity>,<ref_chro>,<query_chro>\n
 * identity = (double)match / (double)align_size in IEEE double precision: u64 -> f64 rounds to nearest even, the division is the
 * correctly rounded one (no fast-math, no reciprocal), 0 / 0 is NaN and x / 0 inf; under no_identity the column is "1.0" and the
 * counters are not read (they may be absent).
 * Plan, scan and fill are the record rows' of wga_text_out.h (k_record_rows_plan<DotplotOvSrc>, ScanItems<DotplotOvFmt>,
 * k_text_items_fill<DotplotOvFmt>).
 *   stage  256 consecutive rows per block are one contiguous stretch, staged in LDS and flushed in 16-byte stores.  A row
 *          without its names is at most 4 x 20 + 24 + 7 = 111 bytes; rows of real files are 40 to 70 bytes (coordinates of up to 9 digits, an identity of 3 to 20 bytes, names of a few letters).  The
 *          stage is 256 x 112 bytes: a block stages its stretch whenever its rows AVERAGE 112 bytes, which leaves a real row 40
 *          bytes and more for longer names, and holds 256 rows of the widest numbers with empty names.  With the 32 bytes of
 *          alignment slack and the fill's two words that is 28 720 bytes of LDS, so that FIVE blocks (20 waves, 5 per SIMD) share
 *          the 160 KiB of a CU (the fill takes 67 VGPRs and no scratch: registers would admit 7).  A thread's work is integer
 *          arithmetic on registers between one read of its head and one write of its row into LDS, so the waves hide each
 *          other's loads, and more of them per CU (a smaller stage) would buy nothing the stage's misses would not cost.  A block whose stretch is longer (names of kilobytes) writes its rows directly.
 * Not tuned past the staged fill: the rows are a few tens of MB against the GB of ops that K1 / K3 read for the counters. */
#define WGA_DOTPLOT_OV_STAGE (WGA_TEXT_ITEMS * 112u)

/* the identity column's bits: the formatter is a function of those */
__device__ __forceinline__ u64 dotplot_ov_identity(u64 match, u64 align_size) {
  const double v = (double)match / (double)align_size;
  u64 b;
  memcpy(&b, &v, 8);
  return b;
}

/* counts == nullptr: no_identity */
template <typename S>
__device__ __forceinline__ void dotplot_ov_row_emit(S& s, const wga_dotplot_ov_head& H, const u8* __restrict__ names, u64 n_name_bytes,
                                                    const wga_cigar_counts* __restrict__ counts, u32 r) {
  const u32 rl = name_span_len(H.rname_off, H.rname_len, n_name_bytes), ql = name_span_len(H.qname_off, H.qname_len, n_name_bytes);
  const u64 a[4] = {H.ref_start, H.ref_end, H.q_first, H.q_second};
#pragma unroll
  for (u32 k = 0; k < 4u; k++) {
    s.dec(a[k]);
    s.c((u8)',');
  }
  if (counts) f64_text_emit(s, dotplot_ov_identity(counts[r].match, H.align_size));
  else s.c((u8)'1'), s.c((u8)'.'), s.c((u8)'0');
  s.c((u8)',');
  csv_field_emit<(u8)','>(s, names + (rl ? H.rname_off : 0u), rl);
  s.c((u8)',');
  csv_field_emit<(u8)','>(s, names + (ql ? H.qname_off : 0u), ql);
  s.c((u8)'\n');
}

/* K34's row source and format (RECORD ROWS in wga_text_out.h): item x is row x of record x */
struct DotplotOvSrc {
  static constexpr u32 kStage = WGA_DOTPLOT_OV_STAGE;
  const u8* names;
  u64 n_name_bytes;
  const wga_dotplot_ov_head* heads;
  const wga_cigar_counts* counts; /* or nullptr: no_identity */
  template <typename S>
  __device__ __forceinline__ void emit(S& s, u32 r) const {
    dotplot_ov_row_emit(s, heads[r], names, n_name_bytes, counts, r);
  }
};
struct DotplotOvFmt : RecordRowsFmt<DotplotOvSrc> {};

#endif /* WGA_K34_DOTPLOT_OVERVIEW_H */
