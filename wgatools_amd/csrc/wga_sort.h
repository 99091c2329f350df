/*
 * wga_sort.h — a stable key sort on the device: an LSD radix sort of n u32 payloads by a u32 key that a functor reads off the
 * payload (K35: the s-line's group number), one counting-sort pass per digit of `bits` bits (1 .. WGA_SORT_MAX_BITS), and only as
 * many passes as the largest key has digits (run_sort_u32 in wga_capi.cpp).  Every pass keeps the order of equal digits, so the
 * whole sort keeps the order of equal keys, whatever the digit width.
 * One pass over blocks of WGA_SORT_ITEMS consecutive items:
 *   hist     k_sort_hist: the block's count of every digit value (LDS atomics) to cnt[digit * n_blocks + block] — digit-major, so
 *            that the exclusive scan of cnt (the shared scan driver, in place) is every (digit, block)'s first place.
 *   scatter  k_sort_scatter: the block walks its items in four rounds of 256 in item order.  In a round the lanes of a wave that
 *            hold the same digit find each other with one ballot per digit bit; the lowest of them leaves their number for the
 *            waves behind, and an item's place is the (digit, block)'s running place + the equal digits of the waves in front +
 *            those of the lanes in front.  Nothing is written at or behind out[n], whatever the scan holds.
 */
#ifndef WGA_SORT_H
#define WGA_SORT_H

#include "wga_kernels.h"

#define WGA_SORT_ITEMS 1024u  /* per block: four rounds of 256 */
#define WGA_SORT_MAX_BITS 8u  /* a digit's width: 256 counters per block */

template <typename K>
__global__ __launch_bounds__(256) void k_sort_hist(K key, const u32* __restrict__ in, u32 n, u32 shift, u32 bits, u32 n_blocks,
                                                   u64* __restrict__ cnt) {
  __shared__ u32 s_h[1u << WGA_SORT_MAX_BITS];
  const u32 tid = threadIdx.x, mask = (1u << bits) - 1u;
  s_h[tid] = 0u;
  __syncthreads();
  for (u32 e = 0; e < 4u; e++) {
    const u64 x = (u64)blockIdx.x * WGA_SORT_ITEMS + e * 256u + tid;
    if (x < (u64)n) atomicAdd(&s_h[(key(in[x]) >> shift) & mask], 1u);
  }
  __syncthreads();
  if (tid <= mask) cnt[(u64)tid * n_blocks + blockIdx.x] = (u64)s_h[tid];
}

template <typename K>
__global__ __launch_bounds__(256) void k_sort_scatter(K key, const u32* __restrict__ in, u32 n, u32 shift, u32 bits, u32 n_blocks,
                                                      const u64* __restrict__ off, u32* __restrict__ out) {
  __shared__ u64 s_run[1u << WGA_SORT_MAX_BITS];   /* the next place of every digit value */
  __shared__ u32 s_w[4][1u << WGA_SORT_MAX_BITS];  /* a round's count of every digit value in each wave */
  const u32 tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6, mask = (1u << bits) - 1u;
  if (tid <= mask) s_run[tid] = off[(u64)tid * n_blocks + blockIdx.x];
  for (u32 w = 0; w < 4u; w++) s_w[w][tid] = 0u;
  __syncthreads();
  for (u32 e = 0; e < 4u; e++) {
    const u64 x = (u64)blockIdx.x * WGA_SORT_ITEMS + e * 256u + tid;
    const bool live = x < (u64)n;
    const u32 v = live ? in[x] : 0u;
    const u32 d = live ? (key(v) >> shift) & mask : 0u;
    u64 peers = __ballot(live); /* the lanes of this wave with this lane's digit */
    for (u32 b = 0; b < bits; b++) {
      const bool one = ((d >> b) & 1u) != 0u;
      const u64 m = __ballot(live && one);
      peers &= one ? m : ~m;
    }
    const u32 rank = (u32)__builtin_popcountll(peers & ((1ull << lane) - 1ull));
    if (live && rank == 0u) s_w[wave][d] = (u32)__builtin_popcountll(peers);
    __syncthreads();
    if (live) {
      u64 pos = s_run[d] + rank;
      for (u32 w = 0; w < wave; w++) pos += s_w[w][d];
      if (pos < (u64)n) out[pos] = v;
    }
    __syncthreads();
    if (tid <= mask) s_run[tid] += (u64)s_w[0][tid] + s_w[1][tid] + s_w[2][tid] + s_w[3][tid];
    for (u32 w = 0; w < 4u; w++) s_w[w][tid] = 0u;
    __syncthreads();
  }
}

/* the bits of the largest key of `count` keys 0 .. count - 1 (0 for one key or none: nothing to sort by) */
static inline unsigned sort_key_bits(unsigned long long count) {
  unsigned b = 0;
  while (b < 32u && (1ull << b) < count) b++;
  return b;
}

#endif /* WGA_SORT_H */
