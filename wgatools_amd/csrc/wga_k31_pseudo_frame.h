/*
 * wga_k31_pseudo_frame.h — K31: everything of a `pafpseudo` file that is not a segment (pseudomaf.rs:98-209: "a score=0\n", the
 * `s` line heads, the target row of N or of the pool, the `-` runs in front of, between and behind a query's segments, the line
 * ends), written around the places K6 fills.
 * One header per kernel family; wga_capi.cpp includes them in dependency order (a header may use helpers of the ones in front of it).
 */
#ifndef WGA_K31_PSEUDO_FRAME_H
#define WGA_K31_PSEUDO_FRAME_H

#include "wga_kernels.h"

/* ============================================================================================ */
/* K31: the row frame writer                                                                    */
/* ============================================================================================ */
/* The text is a list of spans that tile out[0, out_bytes) in order (wga_span_item, include/wga_hip.h): a run of one byte, a copy
 * out of the pool or out of a small text blob, or a hole another kernel writes.  Their lengths run from 0 to 10^8 in one list, so
 * the work is dealt out over OUTPUT BYTES, not over items:
 *   check  one thread per item: the tiling (dst == the end of the item in front, inside out_bytes, the last one ends the text), the
 *          kind, the copy range inside its source; the first bad item by atomicMin.  The items in front of it are a sorted tiling
 *          of out[0, E), E <= out_bytes: all the fill trusts.
 *   fill   one block per tile of WGA_PSEUDO_FRAME_TILE bytes, every thread on its own (no LDS, no barrier).  The block bisects
 *          the items for the one that holds the tile's first byte and the one that holds its last (wave-uniform: scalar loads).
 *          A tile inside ONE item — all but a few, the rows being megabytes — is that item's kind for every 16-byte chunk: nothing
 *          for a hole, a constant store for a run, one unaligned 16-byte load of exactly the chunk's source bytes and a store for a
 *          copy (the load never reaches over the item's source range, so the pool needs no padding).  In any other tile a thread
 *          bisects the tile's items for its chunk's and takes the same path when the chunk lies inside one item; a chunk that
 *          several items share is assembled byte by byte, walking the items forward (items without bytes are stepped over), and
 *          leaves in one 16-byte store unless a hole or the end of the text takes part in it: then its bytes are stored singly,
 *          and the others keep what they held.
 * Every byte of a run or a copy in front of the first bad item is written exactly once and no other byte at all: K6 runs before
 * or after this kernel on the stream. */

__device__ __forceinline__ u64 span_end(const wga_span_item& it) { return it.dst + it.len; }

/* a copy of `len` bytes from `src` lies inside a source of `bytes` bytes */
__device__ __forceinline__ bool span_src_ok(u64 src, u64 len, u64 bytes) { return len <= bytes && src <= bytes - len; }

__global__ __launch_bounds__(256) void k_pseudo_frame_check(u64 n_items, const wga_span_item* __restrict__ items, u64 pool_bytes,
                                                            u64 text_bytes, u64 out_bytes, u64* first_bad) {
  const u64 k = (u64)blockIdx.x * 256u + threadIdx.x;
  if (k >= n_items) return;
  const wga_span_item it = items[k];
  /* an item in front whose end wraps is itself bad (it does not lie inside out_bytes), so the wrapped sum is never the verdict */
  const u64 want = k ? span_end(items[k - 1u]) : 0ull;
  bool bad = it.dst != want || !span_src_ok(it.dst, it.len, out_bytes) || it.kind > WGA_SPAN_HOLE;
  if (it.kind == WGA_SPAN_COPY_POOL) bad = bad || !span_src_ok(it.src, it.len, pool_bytes);
  if (it.kind == WGA_SPAN_COPY_TEXT) bad = bad || !span_src_ok(it.src, it.len, text_bytes);
  if (k + 1u == n_items) bad = bad || span_end(it) != out_bytes;
  if (bad) atomicMin(first_bad, k);
}

/* the largest k in [lo, hi) with items[k].dst <= x, given that items[lo].dst <= x and the dst ascend: the item that holds byte x
 * when x lies in front of the tiling's end (items without bytes share their dst with the item behind them, so the last one with
 * dst <= x is never one of them) */
__device__ __forceinline__ u64 span_find(const wga_span_item* __restrict__ items, u64 lo, u64 hi, u64 x) {
  while (lo + 1u < hi) {
    const u64 mid = lo + ((hi - lo) >> 1);
    if (items[mid].dst <= x) lo = mid; else hi = mid;
  }
  return lo;
}
/* the same for the block's two searches: wave-uniform reads of an array no thread writes */
__device__ __forceinline__ u64 span_find_uniform(const wga_span_item* __restrict__ items, u64 lo, u64 hi, u64 x) {
  while (lo + 1u < hi) {
    const u64 mid = lo + ((hi - lo) >> 1);
    if (WGA_RO64(&items[mid].dst) <= x) lo = mid; else hi = mid;
  }
  return lo;
}

/* the whole chunk out[c, c + 16) lies inside item `it` */
__device__ __forceinline__ void span_chunk_whole(const wga_span_item& it, u64 c, const u8* __restrict__ pool,
                                                 const u8* __restrict__ text, u8* __restrict__ out) {
  if (it.kind == WGA_SPAN_HOLE) return;
  u32x4_a16 v;
  if (it.kind == WGA_SPAN_FILL) {
    const u32 w = ((u32)it.src & 0xFFu) * 0x01010101u;
    v[0] = w, v[1] = w, v[2] = w, v[3] = w;
  } else {
    const u8* s = (it.kind == WGA_SPAN_COPY_POOL ? pool : text) + it.src + (c - it.dst);
    const u32x4_a1 x = *(const u32x4_a1*)s; /* [s, s + 16) is inside the item's source range */
    v[0] = x[0], v[1] = x[1], v[2] = x[2], v[3] = x[3];
  }
  *(u32x4_a16*)(out + c) = v;
}

/* the chunk out[c, ce), ce - c <= 16, whose first byte item k holds: the items are walked forward */
__device__ __forceinline__ void span_chunk_mixed(const wga_span_item* __restrict__ items, u64 k, u64 c, u64 ce,
                                                 const u8* __restrict__ pool, const u8* __restrict__ text, u8* __restrict__ out) {
  wga_span_item it = items[k];
  u64 iend = span_end(it);
  u32 v[4] = {0u, 0u, 0u, 0u}, mask = 0u;
#pragma unroll
  for (u32 j = 0; j < 16u; j++) {
    const u64 p = c + j;
    if (p < ce) {
      while (p >= iend) { /* the tiling reaches ce, so an item that holds p follows */
        it = items[++k];
        iend = span_end(it);
      }
      if (it.kind != WGA_SPAN_HOLE) {
        const u32 b = it.kind == WGA_SPAN_FILL ? ((u32)it.src & 0xFFu)
                                               : (u32)(it.kind == WGA_SPAN_COPY_POOL ? pool : text)[it.src + (p - it.dst)];
        v[j >> 2] |= b << (8u * (j & 3u));
        mask |= 1u << j;
      }
    }
  }
  if (mask == 0xFFFFu) {
    u32x4_a16 x;
    x[0] = v[0], x[1] = v[1], x[2] = v[2], x[3] = v[3];
    *(u32x4_a16*)(out + c) = x;
    return;
  }
#pragma unroll
  for (u32 j = 0; j < 16u; j++)
    if (mask >> j & 1u) WGA_GLOBAL_STORE_U8(out + c + j, (u8)(v[j >> 2] >> (8u * (j & 3u))));
}

/* out is 16-byte aligned; *first_bad is what k_pseudo_frame_check left */
__global__ __launch_bounds__(256) void k_pseudo_frame_fill(u64 n_items, const wga_span_item* __restrict__ items,
                                                           const u8* __restrict__ pool, const u8* __restrict__ text,
                                                           u8* __restrict__ out, const u64* __restrict__ first_bad) {
  const u64 fb = WGA_RO64(first_bad);
  const u64 n_good = fb < n_items ? fb : n_items;
  if (n_good == 0u) return;
  const u64 end = WGA_RO64(&items[n_good - 1u].dst) + WGA_RO64(&items[n_good - 1u].len); /* of the good items' tiling */
  const u64 t0 = (u64)blockIdx.x * WGA_PSEUDO_FRAME_TILE;
  if (t0 >= end) return;
  const u64 t1 = end - t0 > WGA_PSEUDO_FRAME_TILE ? t0 + WGA_PSEUDO_FRAME_TILE : end;
  const u64 i0 = span_find_uniform(items, 0u, n_good, t0), i1 = span_find_uniform(items, i0, n_good, t1 - 1u);
  const u64 c0 = t0 + 16u * threadIdx.x;
  if (i0 == i1) { /* block-uniform */
    const wga_span_item it = items[i0];
    if (it.kind == WGA_SPAN_HOLE) return;
    for (u64 c = c0; c < t1; c += 16u * 256u) {
      if (t1 - c >= 16u)
        span_chunk_whole(it, c, pool, text, out);
      else
        span_chunk_mixed(items, i0, c, t1, pool, text, out);
    }
    return;
  }
  for (u64 c = c0; c < t1; c += 16u * 256u) {
    const u64 k = span_find(items, i0, i1 + 1u, c);
    const wga_span_item it = items[k];
    if (t1 - c >= 16u && span_end(it) - c >= 16u)
      span_chunk_whole(it, c, pool, text, out);
    else
      span_chunk_mixed(items, k, c, t1 - c >= 16u ? c + 16u : t1, pool, text, out);
  }
}

#endif /* WGA_K31_PSEUDO_FRAME_H */
