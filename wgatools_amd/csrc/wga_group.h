/*
 * wga_group.h — group-by on the device: n items, each with a key of bytes, are put into groups of equal keys, and the groups are
 * numbered by their lowest member (first-appearance order).  The algorithm is K24's and K35's (which keep their own copies for now),
 * written once over a key functor K, a plain struct passed by value:
 *   u64  hash(u32 i) const           any function of item i's key: it only places the item in the table
 *   bool same(u32 i, u32 j) const    the keys of items i and j are equal: this alone decides
 * The table has 2^k >= 2 n slots of u64, all ones when empty.  Item i starts at slot hash(i) & hash_mask & slot_mask (hash_mask: a
 * test cuts the hash to a few bits so that every key collides).  Round r = 0, 1, ...:
 *   claim    k_group_claim: every item without a group claims slot start + r (r + 1) / 2 (triangular probing reaches every slot of a
 *            2^k table) with atomicMin((r << 32) | i): a slot taken in an earlier round keeps its owner, one taken in this round
 *            goes to the lowest claimant.
 *   settle   k_group_settle<K>: every such item compares its key with the slot's owner w: equal -> rep[i] = w, otherwise it goes on
 *            the list of round r + 1.  An owner is its own representative; since the lowest claimant wins and all members of a
 *            group walk the same slots, rep[i] is the lowest member of i's group.
 * Then a scan over "rep[i] == i" numbers the groups (ScanGroupRep), and k_group_number gives every item its group's number.
 * The launcher is run_group in wga_capi.cpp.
 */
#ifndef WGA_GROUP_H
#define WGA_GROUP_H

#include "wga_kernels.h"

struct GroupHdr {
  u64 cnt[2]; /* the lengths of the two lists of items without a group: round r reads list r & 1 and appends to the other */
};

/* the slots of a table for n items: a power of two >= 2 n, at least 16, at most 2^32 */
static inline unsigned long long group_slots(unsigned long long n) {
  unsigned long long m = 16;
  while (m < 2 * n && m < (1ull << 32)) m <<= 1;
  return m;
}

__device__ __forceinline__ u32 group_slot(u32 start, u64 r, u32 slot_mask) {
  return (u32)((u64)start + ((r * (r + 1u)) >> 1)) & slot_mask;
}

/* every item i: its start slot, no group yet, a place in list 0 */
template <typename K>
__global__ __launch_bounds__(256) void k_group_init(K key, u64 n, u64 hash_mask, u32 slot_mask, u32* __restrict__ start,
                                                    u32* __restrict__ rep, u32* __restrict__ list) {
  const u64 i = (u64)blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  rep[i] = 0xFFFFFFFFu;
  start[i] = (u32)(key.hash((u32)i) & hash_mask) & slot_mask;
  list[i] = (u32)i;
}

__global__ __launch_bounds__(256) void k_group_claim(const u32* __restrict__ list, u64 m, u64 r, u32 slot_mask,
                                                     const u32* __restrict__ start, u64* __restrict__ slots, GroupHdr* hdr) {
  const u64 x = (u64)blockIdx.x * 256u + threadIdx.x;
  if (x == 0u) hdr->cnt[(r + 1u) & 1u] = 0u; /* the list this round's settle pass appends to */
  if (x >= m) return;
  const u32 i = list[x];
  atomicMin(&slots[group_slot(start[i], r, slot_mask)], (r << 32) | (u64)i);
}

template <typename K>
__global__ __launch_bounds__(256) void k_group_settle(K key, const u32* __restrict__ list, u64 m, u64 n, u64 r, u32 slot_mask,
                                                      const u32* __restrict__ start, const u64* __restrict__ slots,
                                                      u32* __restrict__ rep, u32* __restrict__ next, GroupHdr* hdr) {
  const u64 x = (u64)blockIdx.x * 256u + threadIdx.x;
  if (x >= m) return;
  const u32 i = list[x];
  const u32 w = (u32)slots[group_slot(start[i], r, slot_mask)];
  if ((u64)w < n && key.same(i, w)) { /* the keys decide, never the hash */
    rep[i] = w;
  } else {
    const u64 at = atomicAdd(&hdr->cnt[(r + 1u) & 1u], (u64)1);
    if (at < n) next[at] = i;
  }
}

struct ScanGroupRep { /* scan functor: item i is its group's first */
  const u32* rep;
  __device__ u64 operator()(u32 i) const { return rep[i] == i ? 1u : 0u; }
};

/* group_of[i] = the number of item i's group (gidx = the exclusive scan of ScanGroupRep), order[i] = i.  group_of may be the
 * start slots' array: they are done with. */
__global__ __launch_bounds__(256) void k_group_number(u64 n, const u32* __restrict__ rep, const u64* __restrict__ gidx,
                                                      u32* group_of, u32* __restrict__ order) {
  const u64 i = (u64)blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  const u32 w = rep[i];
  group_of[i] = (u64)w < n ? (u32)gidx[w] : 0u;
  order[i] = (u32)i;
}

#endif /* WGA_GROUP_H */
