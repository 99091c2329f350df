/*
 * wga_k33_stat_rows.h — K33: the TSV rows of `stat --each` (split_final, stat.rs:129-164, written by the csv writer of
 * stat.rs:117-123: tab delimiter, QuoteStyle::Necessary, the f32 columns through ryu) over the per-record statistics of
 * common.rs:116-140.
 * One header per kernel family; wga_capi.cpp includes them in dependency order (a header may use helpers of the ones in front of it).
 */
#ifndef WGA_K33_STAT_ROWS_H
#define WGA_K33_STAT_ROWS_H

#include "wga_text_out.h" /* the sinks, ScanItems, k_text_items_fill and the record rows' skeleton */
#include "wga_paf_head.h" /* csv_field_emit, name_span_len */
#include "wga_f32_text.h" /* f32_text_emit: an f32 as ryu prints it */

/* ============================================================================================ */
/* K33: stat --each row writer                                                                  */
/* ============================================================================================ */
/* Row r of the text is record r, 22 columns:
 *   <ref_name> <ref_size> <ref_start> <query_name> <query_size> <query_start> <aligned_size> 0 <identity> <similarity>
 *   <matched> <mismatched> <ins_event> <del_event> <ins_size> <del_size> <inv_event> <inv_size>
 *   <inv_ins_event> <inv_ins_size> <inv_del_event> <inv_del_size>
 * with tabs between them and "\n" behind.  The sums are mod 2^64, the three f32 columns IEEE single precision: u64 -> f32
 * rounds to nearest even, the division is the correctly rounded one (no fast-math, no reciprocal).
 * Plan, scan and fill are the record rows' of wga_text_out.h (k_record_rows_plan<StatRowSrc>, ScanItems<StatRowsFmt>,
 * k_text_items_fill<StatRowsFmt>).
 *   stage  256 consecutive rows per block are one contiguous stretch, staged in LDS and flushed in 16-byte stores.  A row
 *          without its names is at most 17 x 20 + 3 x 16 + 22 = 410 bytes, but a stage for that many (102.5 KiB) would leave a CU one block; rows of real files are 110 to 140 bytes (names of a few
 *          letters, numbers of up to 9 digits, floats of 9 to 11 bytes: 112 and 115 bytes measured on the two shapes of
 *          profiles/r07_stat_rows_e2e.txt).  The stage is 256 x 156 bytes: with the 32 bytes of alignment slack and the fill's two
 *          words 39 984 bytes of LDS, so that FOUR blocks (16 waves) share the 160 KiB of a CU.  A block whose stretch is longer
 *          (names of kilobytes, or every number at its widest) writes its rows directly. */
#define WGA_STAT_ROWS_STAGE (WGA_TEXT_ITEMS * 156u)

/* the three f32 columns of a record (the bits: the formatter is a function of those) */
struct StatRowF32 {
  u32 identity, similarity, inv_size;
};
__device__ __forceinline__ u32 f32_bits(float f) {
  u32 b;
  memcpy(&b, &f, 4);
  return b;
}
__device__ __forceinline__ StatRowF32 stat_row_f32(const wga_cigar_counts& c, u64 aligned) {
  StatRowF32 f;
  const float a = (float)aligned;
  f.identity = f32_bits((float)c.match / a);
  f.similarity = f32_bits((float)(c.match + c.mismatch) / a);
  const u64 query_align = c.match + c.mismatch + c.ins_bp + c.inv_ins_bp;
  f.inv_size = c.inv_ev != 0u ? f32_bits((float)(aligned + query_align) / (float)(c.inv_ev + 1u)) : 0u;
  return f;
}

/* kPair: a row of the merged table (K36, StatPairRowSrc in wga_k36_stat_pairs.h): c holds a pair's sums, column 8 is ref_size -
 * aligned_size (mod 2^64, stat.rs:216) and column 18 the f32 with the bits inv_bits, the fold over the pair's records */
template <bool kPair = false, typename S>
__device__ __forceinline__ void stat_row_emit(S& s, const wga_stat_row_head& H, const u8* __restrict__ names, u64 n_name_bytes,
                                              const wga_cigar_counts& c, u32 inv_bits = 0u) {
  const u32 rl = name_span_len(H.rname_off, H.rname_len, n_name_bytes), ql = name_span_len(H.qname_off, H.qname_len, n_name_bytes);
  const u64 aligned = c.match + c.mismatch + c.del_bp + c.inv_del_bp;
  const StatRowF32 f = stat_row_f32(c, aligned);
  csv_field_emit<(u8)'\t'>(s, names + (rl ? H.rname_off : 0u), rl);
  s.c((u8)'\t');
  s.dec(H.ref_size);
  s.c((u8)'\t');
  s.dec(H.ref_start);
  s.c((u8)'\t');
  csv_field_emit<(u8)'\t'>(s, names + (ql ? H.qname_off : 0u), ql);
  s.c((u8)'\t');
  s.dec(H.query_size);
  s.c((u8)'\t');
  s.dec(H.query_start);
  s.c((u8)'\t');
  s.dec(aligned);
  s.c((u8)'\t');
  if (kPair) s.dec(H.ref_size - aligned);
  else s.c((u8)'0'); /* unaligned_size: split_final leaves it 0 */
  s.c((u8)'\t');
  f32_text_emit(s, f.identity);
  s.c((u8)'\t');
  f32_text_emit(s, f.similarity);
  s.c((u8)'\t');
  const u64 a[7] = {c.match, c.mismatch, c.ins_ev, c.del_ev, c.ins_bp, c.del_bp, c.inv_ev};
#pragma unroll
  for (u32 k = 0; k < 7u; k++) {
    s.dec(a[k]);
    s.c((u8)'\t');
  }
  f32_text_emit(s, kPair ? inv_bits : f.inv_size);
  const u64 b[4] = {c.inv_ins_ev, c.inv_ins_bp, c.inv_del_ev, c.inv_del_bp};
#pragma unroll
  for (u32 k = 0; k < 4u; k++) {
    s.c((u8)'\t');
    s.dec(b[k]);
  }
  s.c((u8)'\n');
}

/* K33's row source and format (RECORD ROWS in wga_text_out.h): item x is row x of record x */
struct StatRowSrc {
  static constexpr u32 kStage = WGA_STAT_ROWS_STAGE;
  const u8* names;
  u64 n_name_bytes;
  const wga_stat_row_head* heads;
  const wga_cigar_counts* counts;
  template <typename S>
  __device__ __forceinline__ void emit(S& s, u32 r) const {
    stat_row_emit(s, heads[r], names, n_name_bytes, counts[r]);
  }
};
struct StatRowsFmt : RecordRowsFmt<StatRowSrc> {};

#endif /* WGA_K33_STAT_ROWS_H */
