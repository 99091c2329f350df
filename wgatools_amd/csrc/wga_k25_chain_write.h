/*
 * wga_k25_chain_write.h — K25: the chain record writer of `filter -f chain` (chain.rs:92-100,185-204 behind the selection of
 * tools/filter.rs:17-39,91-105).
 * One header per kernel family; wga_capi.cpp includes them in dependency order (a header may use helpers of the ones in front of it).
 */
#ifndef WGA_K25_CHAIN_WRITE_H
#define WGA_K25_CHAIN_WRITE_H

#include "wga_text_out.h"        /* the sinks, ScanItems and k_text_items_fill */
#include "wga_chain_items.h"     /* ChainItemBase: the item numbering */
#include "wga_k23_chain_split.h" /* wga_chain_head_dev */

/* ============================================================================================ */
/* K25: chain record writer                                                                     */
/* ============================================================================================ */
/* The text of the kept chains is ONE contiguous byte stream, so it is written as a stream of ITEMS in file order, numbered as
 * wga_chain_items.h says.  A head item is the header line without its newline ("chain\t<score>\t<tname>\t...\t<id>"), a line
 * item is "\n<size>\t<col2>\t<col3>"; the item that ends a chain also carries the "\n\n" behind it.  Items of dropped chains
 * have size 0.
 *   plan   one thread per chain: the keep flag (filter.rs:96-101, both compare with `<`, the span wraps) and the head's byte
 *          count (0 = dropped; a kept head has at least 30 bytes), the kept chains counted by one atomicAdd per block.
 *   scan   the exclusive scan of the item sizes (ScanItems<ChainWriteFmt>: an item's chain by bisection in line_off[r] + r).
 *   fill   k_text_items_fill<ChainWriteFmt> (wga_text_out.h): 256 consecutive items per block, staged and flushed as that file
 *          describes.  256 line items are at most 256 x 65 bytes: that is the stage.  A block whose stretch is longer (a head
 *          with names of kilobytes) writes its items directly.  kCheckSize is off: an item's span is checked, its size is not.
 * The emitters run into a TextCount for the plan and the scan, into a TextPut for the fill. */
#define WGA_CHAIN_WRITE_STAGE (WGA_TEXT_ITEMS * 65u)

struct wga_chain_filter_params_dev {
  u64 min_block_size, min_query_size;
};

/* chain.rs:185-204: the score (1 to 15 digits for a file K23 takes: its f64 Display is the plain decimal), names as they are */
template <typename S>
__device__ __forceinline__ void chain_head_emit(S& s, const wga_chain_head_dev& H, const u8* __restrict__ text) {
  const char* c = "chain\t";
  for (u32 k = 0; k < 6u; k++) s.c((u8)c[k]);
  s.dec(H.num[0]);
  s.c((u8)'\t');
  s.str(text + H.tname_off, H.tname_len);
  s.c((u8)'\t');
  s.dec(H.num[1]);
  s.c((u8)'\t');
  s.c(H.tstrand_neg ? (u8)'-' : (u8)'+');
  s.c((u8)'\t');
  s.dec(H.num[2]);
  s.c((u8)'\t');
  s.dec(H.num[3]);
  s.c((u8)'\t');
  s.str(text + H.qname_off, H.qname_len);
  s.c((u8)'\t');
  s.dec(H.num[4]);
  s.c((u8)'\t');
  s.c(H.qstrand_neg ? (u8)'-' : (u8)'+');
  s.c((u8)'\t');
  s.dec(H.num[5]);
  s.c((u8)'\t');
  s.dec(H.num[6]);
  s.c((u8)'\t');
  s.dec(H.num[7]);
}
/* chain.rs:92-100: always three columns */
template <typename S>
__device__ __forceinline__ void chain_line_emit(S& s, const u64* __restrict__ v) {
  const u64 a = v[0], b = v[1], c = v[2]; /* all three before the first byte is written */
  s.c((u8)'\n');
  s.dec(a);
  s.c((u8)'\t');
  s.dec(b);
  s.c((u8)'\t');
  s.dec(c);
}
template <typename S>
__device__ __forceinline__ void chain_end_emit(S& s) {
  s.c((u8)'\n');
  s.c((u8)'\n');
}

/* plan[r] = the bytes of chain r's head item without a chain end, 0 when the chain is dropped; *n_kept += the kept chains */
__global__ __launch_bounds__(256) void k_chain_write_plan(const u8* __restrict__ text,
                                                          const wga_chain_head_dev* __restrict__ heads, u32 n_chains,
                                                          wga_chain_filter_params_dev P, u64* __restrict__ plan, u64* n_kept) {
  __shared__ u64 s_w[5];
  const u64 r = (u64)blockIdx.x * 256u + threadIdx.x;
  u64 kept = 0;
  if (r < (u64)n_chains) {
    const wga_chain_head_dev H = heads[r];
    const bool keep = !(H.num[3] - H.num[2] < P.min_block_size || H.num[4] < P.min_query_size);
    TextCount c;
    if (keep) chain_head_emit(c, H, text);
    plan[r] = c.n;
    kept = keep ? 1u : 0u;
  }
  u64 tot;
  (void)block_excl_scan_u64(kept, s_w, &tot);
  if (threadIdx.x == 0 && tot) atomicAdd(n_kept, tot);
}

/* K25's format: every item of a dropped chain (plan[r] == 0) has no bytes */
struct ChainWriteFmt : ChainItemBase {
  static constexpr u32 kStage = WGA_CHAIN_WRITE_STAGE;
  static constexpr bool kCheckSize = false;
  const u8* text;
  const wga_chain_head_dev* heads;
  template <typename S>
  __device__ __forceinline__ void head_emit(S& s, u32 r) const { chain_head_emit(s, heads[r], text); }
  template <typename S>
  __device__ __forceinline__ void line_emit(S& s, u64 l, u32) const { chain_line_emit(s, lines + 3u * l); }
  template <typename S>
  __device__ __forceinline__ void end_emit(S& s) const { chain_end_emit(s); }
  __device__ __forceinline__ u64 size(u64 x, u32 r) const {
    const u64 head = plan[r]; /* read with the chain's offsets, not behind them */
    const ChainItem i = chain_item(*this, x, r);
    return head == 0u ? 0u : chain_item_size(*this, i, r, head);
  }
  template <typename S>
  __device__ __forceinline__ void emit(S& s, u64 x, u32 r) const { chain_item_emit(*this, s, x, r); }
};

#endif /* WGA_K25_CHAIN_WRITE_H */
