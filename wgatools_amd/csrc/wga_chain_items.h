/* wga_chain_items.h — what kernels over chain records share: the items of a stream of chains (K25's and K27's formats derive from
 * ChainItemBase; so does K28's, with a MAF block's runs in place of a chain's data lines) and a data line's part of chain2paf's CIGAR text (K11 and K27). */
#ifndef WGA_CHAIN_ITEMS_H
#define WGA_CHAIN_ITEMS_H

#include "wga_text_out.h" /* the sinks, csr_find_in */

/* chain2paf's CIGAR text of one data line (cigar.rs:576-610): "<size>M" always, the 3rd column as I and the 2nd as D when
 * non-zero.  v = the line's three values, all read before the first byte is written (one wait for memory, not one per column) */
template <typename S>
__device__ __forceinline__ void c2p_line_emit(S& s, const u64* __restrict__ v) {
  const u64 m = v[0], d = v[1], i = v[2];
  s.dec(m);
  s.c((u8)'M');
  if (i) {
    s.dec(i);
    s.c((u8)'I');
  }
  if (d) {
    s.dec(d);
    s.c((u8)'D');
  }
}

/* The items of a stream of chains in file order, whatever their text: the head of chain r is item line_off[r] + r, data line l
 * of chain r is item l + r + 1 (so the chain of item x is the largest r with line_off[r] + r <= x), and the item that ends a chain
 * (its last line, or the head of a chain without lines) also carries the format's end.  n_lines bounds the data-line index for
 * offsets that are not a splitter's. */
struct ChainItemBase {
  const u64* lines;
  const u64* line_off;
  const u64* plan; /* per chain: the bytes of its head item without the chain's end */
  u32 n_rec;       /* chains */
  u64 n_lines;
  __device__ __forceinline__ u32 rec(u64 x, u32 lo, u32 hi) const { return csr_find_in(line_off, lo, hi, x, true); }
};
struct ChainItem {
  u64 l;     /* the data line, when it is one */
  bool head; /* the chain's head */
  bool none; /* a data line that does not exist: no bytes */
  bool last; /* it ends its chain */
};
__device__ __forceinline__ ChainItem chain_item(const ChainItemBase& it, u64 x, u32 r) {
  const u64 first = it.line_off[r], end = it.line_off[r + 1u];
  ChainItem i;
  i.head = x == first + (u64)r;
  i.l = x - (u64)r - 1u;
  i.none = !i.head && i.l >= it.n_lines;
  i.last = i.head ? first == end : i.l + 1u == end;
  return i;
}
/* item i of chain r of a format F over ChainItemBase with head_emit(s, r), line_emit(s, l, r) and end_emit(s): its bytes (`head`
 * = the plan's bytes of r's head: names are read once), and its text */
template <typename F>
__device__ __forceinline__ u64 chain_item_size(const F& f, const ChainItem& i, u32 r, u64 head) {
  if (i.none) return 0u;
  TextCount c;
  if (i.head) c.n = head; else f.line_emit(c, i.l, r);
  if (i.last) f.end_emit(c);
  return c.n;
}
template <typename F, typename S>
__device__ __forceinline__ void chain_item_emit(const F& f, S& s, u64 x, u32 r) {
  const ChainItem i = chain_item(f, x, r);
  if (i.none) return;
  if (i.head) f.head_emit(s, r); else f.line_emit(s, i.l, r);
  if (i.last) f.end_emit(s);
}

#endif /* WGA_CHAIN_ITEMS_H */
