/*
 * wga_k28_maf2paf.h — K28: the PAF record writer of `maf2paf` (the record of maf.rs:484-520, written by the csv writer of
 * converter.rs:29-54: tab delimiter, QuoteStyle::Necessary).
 * One header per kernel family; wga_capi.cpp includes them in dependency order (a header may use helpers of the ones in front of it).
 */
#ifndef WGA_K28_MAF2PAF_H
#define WGA_K28_MAF2PAF_H

#include "wga_text_out.h"    /* the sinks, ScanItems and k_text_items_fill */
#include "wga_chain_items.h" /* ChainItemBase: the item numbering, with K3's runs in place of data lines */
#include "wga_paf_head.h"    /* csv_field_emit, paf_head_emit: a record's columns */
#include "wga_k11_bridges.h" /* MafRunSrc, maf_run_emit: a run's part of the cg:Z: text */

/* ============================================================================================ */
/* K28: maf2paf record writer                                                                   */
/* ============================================================================================ */
/* One PAF record per block, the records back to back: ONE contiguous byte stream, written as a stream of ITEMS in block order,
 * numbered as wga_chain_items.h says with a block's K3 runs where a chain has data lines: the head of block r is item
 * run_off[r] + r, run x of block r is item x + r + 1.  A head item is the twelve columns and the two tags' names
 * ("<qname>\t...\t255\tNM:i:<n>\tcg:Z:"), a run item is "<length><=|I|D|X>" as K11's wga_maf_runs_cigar_text prints it (the same
 * emitter: 19 digits at the most for K3's ascending starts, which are a u64 >> 3, and the letter; 20 digits where arrays that
 * are not K3's make the difference wrap); the item that ends a block also carries the "\n".
 *   plan   one thread per block: matches and block_length from K3's counters (mod 2^64) and the head's byte count, kept for
 *          the fill.
 *   scan   the exclusive scan of the item sizes (ScanItems<Maf2PafFmt>: an item's block by bisection in run_off[r] + r).
 *   fill   k_text_items_fill<Maf2PafFmt> (wga_text_out.h): 256 consecutive items per block.  256 run items are at most
 *          256 x 21 bytes (22 with a wrapped length): the stage is 256 x 24 (6 KiB + 32).  A block whose stretch is longer (a head with names of
 *          kilobytes) writes its items directly.  kCheckSize is off, as in K25 and K27. */
#define WGA_M2P_STAGE (WGA_TEXT_ITEMS * 24u)

/* = wga_maf2paf_head (wga_hip.h) in the kernels' types */
struct wga_maf2paf_head_dev {
  u64 q[3], t[3];
  u64 qname_off, tname_off;
  u32 qname_len, tname_len;
  u8 strand_neg, pad[7];
};

/* maf.rs:484-520: the record's columns from the caller's numbers and the block's two sums.  A name span that does not lie inside
 * the name buffer is empty. */
template <typename S>
__device__ __forceinline__ void m2p_head_emit(S& s, const wga_maf2paf_head_dev& H, const u8* __restrict__ names, u64 n_name_bytes,
                                              u64 matches, u64 block_length) {
  const u32 ql = name_span_len(H.qname_off, H.qname_len, n_name_bytes), tl = name_span_len(H.tname_off, H.tname_len, n_name_bytes);
  paf_head_emit<true>(s, names + (ql ? H.qname_off : 0u), ql, H.q, H.strand_neg != 0, names + (tl ? H.tname_off : 0u), tl, H.t,
                      matches, block_length, 255u);
}

/* per block r: sums[2 r] = matches, sums[2 r + 1] = block_length, plan[r] = the bytes of its head item without the record's end */
__global__ __launch_bounds__(256) void k_maf2paf_plan(const u8* __restrict__ names, u64 n_name_bytes,
                                                      const wga_maf2paf_head_dev* __restrict__ heads, u32 n,
                                                      const wga_cigar_counts* __restrict__ counts, u64* __restrict__ plan,
                                                      u64* __restrict__ sums) {
  const u64 r = (u64)blockIdx.x * 256u + threadIdx.x;
  if (r >= (u64)n) return;
  const wga_cigar_counts c = counts[r];
  const u64 matches = c.match;
  const u64 block_length = c.match + c.mismatch + c.ins_bp + c.inv_ins_bp + c.del_bp + c.inv_del_bp;
  TextCount t;
  m2p_head_emit(t, heads[r], names, n_name_bytes, matches, block_length);
  plan[r] = t.n;
  sums[2u * r] = matches;
  sums[2u * r + 1u] = block_length;
}

/* K28's format over the chain items' numbering: `lines` = K3's runs, `line_off` = their offsets, `n_lines` = their number */
struct Maf2PafFmt : ChainItemBase {
  static constexpr u32 kStage = WGA_M2P_STAGE;
  static constexpr bool kCheckSize = false;
  const u8* names;
  u64 n_name_bytes;
  const wga_maf2paf_head_dev* heads;
  const u64* sums;
  const u64* cols;
  template <typename S>
  __device__ __forceinline__ void head_emit(S& s, u32 r) const {
    m2p_head_emit(s, heads[r], names, n_name_bytes, sums[2u * (u64)r], sums[2u * (u64)r + 1u]);
  }
  template <typename S>
  __device__ __forceinline__ void line_emit(S& s, u64 x, u32 r) const {
    MafRunSrc m;
    m.runs = lines;
    m.run_off = line_off;
    m.cols = cols;
    maf_run_emit(s, m, x, r);
  }
  template <typename S>
  __device__ __forceinline__ void end_emit(S& s) const { s.c((u8)'\n'); }
  __device__ __forceinline__ u64 size(u64 x, u32 r) const { return chain_item_size(*this, chain_item(*this, x, r), r, plan[r]); }
  template <typename S>
  __device__ __forceinline__ void emit(S& s, u64 x, u32 r) const { chain_item_emit(*this, s, x, r); }
};

#endif /* WGA_K28_MAF2PAF_H */
