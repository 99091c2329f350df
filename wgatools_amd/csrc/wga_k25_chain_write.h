/*
 * wga_k25_chain_write.h — K25: the chain record writer of `filter -f chain` (chain.rs:92-100,185-204 behind the selection of
 * tools/filter.rs:17-39,91-105).
 * One header per kernel family; wga_capi.cpp includes them in dependency order (a header may use helpers of the ones in front of it).
 */
#ifndef WGA_K25_CHAIN_WRITE_H
#define WGA_K25_CHAIN_WRITE_H

#include "wga_text_out.h"        /* the sinks, TextStretch, csr_find_in */
#include "wga_k23_chain_split.h" /* wga_chain_head_dev */

/* ============================================================================================ */
/* K25: chain record writer                                                                     */
/* ============================================================================================ */
/* The text of the kept chains is ONE contiguous byte stream, so it is written as a stream of ITEMS in file order: the head of
 * chain 0, its data lines, the head of chain 1, its data lines, ...  The head of chain r is item line_off[r] + r, data line l
 * of chain r is item l + r + 1.  A head item is the header line without its newline ("chain\t<score>\t<tname>\t...\t<id>"), a
 * line item is "\n<size>\t<col2>\t<col3>"; the item that ends a chain (its last line, or the head of a chain without lines)
 * also carries the "\n\n" behind the chain.  Items of dropped chains have size 0.
 *   plan   one thread per chain: the keep flag (filter.rs:96-101, both compare with `<`, the span wraps) and the head's byte
 *          count (0 = dropped; a kept head has at least 30 bytes), the kept chains counted by one atomicAdd per block.
 *   scan   the exclusive scan of the item sizes (ScanChainItem: an item's chain by bisection in line_off[r] + r).
 *   fill   256 consecutive items per block = one contiguous stretch of the text, whatever record borders lie inside it, staged
 *          and flushed as wga_text_out.h describes.  256 line items are at most 256 x 65 bytes: that is the stage.  A block whose
 *          stretch is longer (a head with names of kilobytes) writes its items directly.
 * The chain of item x is csr_find_in(line_off, lo, hi, x, true): the largest r with line_off[r] + r <= x.  The emitters run into a
 * TextCount for the plan and the scan, into a TextPut for the fill. */
#define WGA_CHAIN_WRITE_ITEMS 256u
#define WGA_CHAIN_WRITE_STAGE (WGA_CHAIN_WRITE_ITEMS * 65u)

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
  s.c((u8)'\n');
  s.dec(v[0]);
  s.c((u8)'\t');
  s.dec(v[1]);
  s.c((u8)'\t');
  s.dec(v[2]);
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
    c.n = 0;
    if (keep) chain_head_emit(c, H, text);
    plan[r] = c.n;
    kept = keep ? 1u : 0u;
  }
  u64 tot;
  (void)block_excl_scan_u64(kept, s_w, &tot);
  if (threadIdx.x == 0 && tot) atomicAdd(n_kept, tot);
}

/* item x of chain r: its bytes.  n_lines bounds the data-line index for offsets that are not a splitter's */
struct ChainItems {
  const u64* lines;
  const u64* line_off;
  const u64* plan;
  u32 n_chains;
  u64 n_lines;
  __device__ __forceinline__ u64 size(u64 x, u32 r) const {
    const u64 head = plan[r];
    if (head == 0u) return 0u;
    const u64 first = line_off[r], end = line_off[r + 1u];
    if (x == first + (u64)r) return head + (first == end ? 2u : 0u);
    const u64 l = x - (u64)r - 1u;
    if (l >= n_lines) return 0u;
    TextCount c;
    c.n = 0;
    chain_line_emit(c, lines + 3u * l);
    return c.n + (l + 1u == end ? 2u : 0u);
  }
};
struct ScanChainItem { /* scan functor: the bytes of item x */
  ChainItems it;
  __device__ u64 operator()(u32 x) const { return it.size((u64)x, csr_find_in(it.line_off, 0u, it.n_chains, (u64)x, true)); }
};

/* items [256 b, 256 b + 256) of n_items; isc = the exclusive scan of their sizes (isc[n_items] = the text's length).  Nothing is
 * written outside out[0, total): a block whose stretch ends behind `total` (a scan that is not this call's) writes nothing. */
__global__ __launch_bounds__(256) void k_chain_write_fill(ChainItems it, u64 n_items, const u8* __restrict__ text,
                                                          const wga_chain_head_dev* __restrict__ heads,
                                                          const u64* __restrict__ isc, u64 total, u8* __restrict__ out) {
  __shared__ u32x4_a16 s_buf[(WGA_CHAIN_WRITE_STAGE + 32u) / 16u];
  __shared__ u32 s_r[2];
  const u32 tid = threadIdx.x;
  const u64 x0 = (u64)blockIdx.x * WGA_CHAIN_WRITE_ITEMS;
  const u64 x1 = x0 + WGA_CHAIN_WRITE_ITEMS < n_items ? x0 + WGA_CHAIN_WRITE_ITEMS : n_items;
  const u64 e0 = isc[x0], e1 = isc[x1]; /* bytes in front of the block, and behind it */
  if (e1 <= e0 || e1 > total) return;   /* block-uniform: every chain of the block is dropped */
  if (tid < 2u) s_r[tid] = csr_find_in(it.line_off, 0u, it.n_chains, tid ? x1 - 1u : x0, true);
  __syncthreads();
  const TextStretch st(s_buf, WGA_CHAIN_WRITE_STAGE, out + e0, e1 - e0); /* block-uniform */
  const u64 x = x0 + tid;
  if (x < x1) {
    const u64 at = isc[x], sz = isc[x + 1u] - at;
    if (sz) { /* a kept chain's item */
      const u32 r = csr_find_in(it.line_off, s_r[0], s_r[1] + 1u, x, true);
      TextPut w;
      w.p = st.at(at - e0);
      const u64 first = it.line_off[r], end = it.line_off[r + 1u];
      if (x == first + (u64)r) {
        chain_head_emit(w, heads[r], text);
        if (first == end) chain_end_emit(w);
      } else {
        const u64 l = x - (u64)r - 1u;
        chain_line_emit(w, it.lines + 3u * l);
        if (l + 1u == end) chain_end_emit(w);
      }
    }
  }
  st.flush_block(tid);
}

#endif /* WGA_K25_CHAIN_WRITE_H */
