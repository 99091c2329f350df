/*
 * wga_k27_chain2paf.h — K27: the PAF record writer of `chain2paf` (convert2paf chain.rs:430-452 over parse_chain_to_cigar
 * cigar.rs:554-627, written by the csv writer of converter.rs:391-416: tab delimiter, QuoteStyle::Necessary).
 * One header per kernel family; wga_capi.cpp includes them in dependency order (a header may use helpers of the ones in front of it).
 */
#ifndef WGA_K27_CHAIN2PAF_H
#define WGA_K27_CHAIN2PAF_H

#include "wga_text_out.h"         /* the sinks, ScanItems and k_text_items_fill */
#include "wga_k23_chain_split.h"  /* wga_chain_head_dev */
#include "wga_chain_items.h"      /* ChainItemBase: the item numbering; c2p_line_emit: a data line's part of the CIGAR text */
#include "wga_paf_head.h"         /* csv_field_emit, paf_head_emit: a record's columns */

/* ============================================================================================ */
/* K27: chain2paf record writer                                                                 */
/* ============================================================================================ */
/* One PAF record per chain, the records back to back: ONE contiguous byte stream, written as a stream of ITEMS in file order,
 * numbered as wga_chain_items.h says.  A head item is the twelve columns and the tag's name ("<qname>\t...\t255\tcg:Z:"), a line
 * item is the line's part of the CIGAR text ("<size>M", "<col3>I" and "<col2>D" when non-zero: at most 63 bytes); the item that
 * ends a chain also carries the record's "\n".
 *   sums   columns 10 and 11 need no op walk (mismatch is 0, a deletion counts once whichever strand books it): matches = the
 *          sum of the chain's sizes, block_length = matches + the sum of its 2nd columns, both mod 2^64.  Two wrapping exclusive
 *          scans over ALL data lines (the context's scan driver), a chain's sums are differences of them: no thread's work
 *          depends on a chain's length.
 *   plan   one thread per chain: the two sums and the head's byte count, kept for the fill.
 *   scan   the exclusive scan of the item sizes (ScanItems<Chain2PafFmt>: an item's chain by bisection in line_off[r] + r).
 *   fill   k_text_items_fill<Chain2PafFmt> (wga_text_out.h): 256 consecutive items per block, staged and flushed as that file
 *          describes.  256 line items are at most 256 x 64 bytes: that is the stage (16 KiB + 32: nine blocks' worth fit a CU's
 *          160 KiB, so the LDS does not bound the occupancy of 256-thread blocks; it leaves in 16-byte stores).  A block whose
 *          stretch is longer (a head with names of kilobytes) writes its items directly.  kCheckSize is off, as in K25.
 * The emitters run into a TextCount for the plan and the scan, into a TextPut for the fill. */
#define WGA_C2P_STAGE (WGA_TEXT_ITEMS * 64u)

/* chain.rs:436-451: the query's columns are num[4 .. 6], the target's num[1 .. 3]; the target's strand is not printed.  A name
 * span that does not lie inside the text (arrays that are not a splitter's) is empty. */
template <typename S>
__device__ __forceinline__ void c2p_head_emit(S& s, const wga_chain_head_dev& H, const u8* __restrict__ text, u64 n_bytes,
                                              u64 matches, u64 block_length) {
  const u32 ql = name_span_len(H.qname_off, H.qname_len, n_bytes), tl = name_span_len(H.tname_off, H.tname_len, n_bytes);
  paf_head_emit(s, text + (ql ? H.qname_off : 0u), ql, H.num + 4, H.qstrand_neg != 0, text + (tl ? H.tname_off : 0u), tl, H.num + 1,
                matches, block_length, 255u);
}
/* scan functor: column `col` of data line x (the sums wrap) */
struct ScanChainCol {
  const u64* lines;
  u32 col;
  __device__ u64 operator()(u32 x) const { return lines[3u * (u64)x + col]; }
};

/* per chain r: sums[2 r] = matches, sums[2 r + 1] = block_length, plan[r] = the bytes of its head item without the record's end.
 * ps / pd = the exclusive scans of the sizes and of the 2nd columns over the n_lines data lines (n_lines + 1 entries each). */
__global__ __launch_bounds__(256) void k_chain2paf_plan(const u8* __restrict__ text, u64 n_bytes,
                                                        const wga_chain_head_dev* __restrict__ heads, u32 n_chains,
                                                        const u64* __restrict__ line_off, u64 n_lines, const u64* __restrict__ ps,
                                                        const u64* __restrict__ pd, u64* __restrict__ plan, u64* __restrict__ sums) {
  const u64 r = (u64)blockIdx.x * 256u + threadIdx.x;
  if (r >= (u64)n_chains) return;
  u64 a = line_off[r], b = line_off[r + 1u];
  a = a < n_lines ? a : n_lines; /* offsets that are not a splitter's stay inside the scans */
  b = b < n_lines ? b : n_lines;
  const u64 matches = ps[b] - ps[a], block_length = matches + (pd[b] - pd[a]);
  TextCount c;
  c2p_head_emit(c, heads[r], text, n_bytes, matches, block_length);
  plan[r] = c.n;
  sums[2u * r] = matches;
  sums[2u * r + 1u] = block_length;
}

/* K27's format over the chain items' numbering: the head's columns need the chain's two sums */
struct Chain2PafFmt : ChainItemBase {
  static constexpr u32 kStage = WGA_C2P_STAGE;
  static constexpr bool kCheckSize = false;
  const u8* text;
  u64 n_bytes;
  const wga_chain_head_dev* heads;
  const u64* sums;
  template <typename S>
  __device__ __forceinline__ void head_emit(S& s, u32 r) const {
    c2p_head_emit(s, heads[r], text, n_bytes, sums[2u * (u64)r], sums[2u * (u64)r + 1u]);
  }
  template <typename S>
  __device__ __forceinline__ void line_emit(S& s, u64 l, u32) const { c2p_line_emit(s, lines + 3u * l); }
  template <typename S>
  __device__ __forceinline__ void end_emit(S& s) const { s.c((u8)'\n'); }
  __device__ __forceinline__ u64 size(u64 x, u32 r) const { return chain_item_size(*this, chain_item(*this, x, r), r, plan[r]); }
  template <typename S>
  __device__ __forceinline__ void emit(S& s, u64 x, u32 r) const { chain_item_emit(*this, s, x, r); }
};

#endif /* WGA_K27_CHAIN2PAF_H */
