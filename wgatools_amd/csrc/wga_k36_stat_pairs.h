/*
 * wga_k36_stat_pairs.h — K36: the merged table of `stat` (merge_final_from_pair, stat.rs:167-223): the records of a piece grouped
 * into pairs (ref_name, ref_size, query_name, query_size), the eleven counters summed and the two starts' minima taken per pair,
 * inv_size folded in record order, and the pairs' rows through K33's row writer.
 * One header per kernel family; wga_capi.cpp includes them in dependency order (a header may use helpers of the ones in front of it).
 * wga_stat_pairs, passes of the first call:
 *   groups    wga_group.h over StatPairKey: the hash places a record, the name bytes and the two sizes decide.  Pairs are numbered
 *             by their lowest record.
 *   sort      wga_sort.h: the records arranged by pair number, input order within a pair.
 *   bounds    k_stat_pairs_bounds: a pair's first sorted place, gstart[g] (gstart[n_pairs] = n).
 *   inverted  a scan over "sorted place p holds a record with inv_ev != 0", and k_stat_pairs_inv_vals: those records' f32 inv_size
 *             values (stat_row_f32) back to back in sorted order, so that a pair's are inv_val[invsc[gstart[g]] .. invsc[gstart[g + 1]]).
 * and of the second call:
 *   init      k_stat_pairs_init: first_rec, n_recs, the minima's start values (the sizes, stat.rs:186-189), zero sums.
 *   reduce    k_stat_pairs_reduce: 256 consecutive sorted places per block.  A wave that holds one pair only (the rule: a file is
 *             often a single pair) adds up with shuffles and one lane carries the wave's sums into the block's LDS accumulators,
 *             any other wave's lanes add there themselves.  The block then hands every pair it saw to memory: a pair whose run lies
 *             inside the block by plain stores, one that crosses a block border by u64 atomicAdd / atomicMin, which are order-free
 *             for integers.  No global atomic per record.
 *   fold      k_stat_pairs_fold: one wave per pair; 64 values per load, added in lane order into the accumulator that starts from
 *             d_inv_in[g] (or +0.0): the left fold of stat.rs:206 over the pair's inverted records.  A repeat of the second call
 *             runs this pass alone.
 */
#ifndef WGA_K36_STAT_PAIRS_H
#define WGA_K36_STAT_PAIRS_H

#include "wga_group.h"
#include "wga_sort.h"
#include "wga_k33_stat_rows.h" /* stat_row_f32, stat_row_emit, name_span_len */

struct K36Hdr {
  GroupHdr g;
  u64 n, n_pairs;   /* what the first call grouped, and into how many pairs */
  u64 where;        /* which of the sort's two buffers holds the sorted order */
  u64 filled[2];    /* the d_pairs and d_pair_of_rec the second call has written already (0: none) */
  u64 pad;
};

struct wga_stat_pair_dev { /* = wga_stat_pair (include/wga_hip.h), in the kernels' own types */
  u64 first_rec, n_recs, ref_start, query_start;
  u64 sum[11]; /* wga_cigar_counts order */
  u32 inv_size_bits, pad;
};

/* the key of a record: both names' bytes (a span outside the buffer is the empty name) and the two sizes */
struct StatPairKey {
  const u8* names;
  u64 n_name_bytes;
  const wga_stat_row_head* heads;
  /* FNV-1a over ref_name, its length, query_name and the sizes; then a finaliser, so that the low bits (which pick the slot)
   * depend on every byte */
  __device__ __forceinline__ u64 hash(u32 i) const {
    const wga_stat_row_head& H = heads[i];
    const u32 rl = name_span_len(H.rname_off, H.rname_len, n_name_bytes), ql = name_span_len(H.qname_off, H.qname_len, n_name_bytes);
    u64 h = 0xCBF29CE484222325ull;
    for (u32 k = 0; k < rl; k++) h = (h ^ names[H.rname_off + k]) * 0x100000001B3ull;
    h = (h ^ (u64)rl ^ 0xFF00u) * 0x100000001B3ull;
    for (u32 k = 0; k < ql; k++) h = (h ^ names[H.qname_off + k]) * 0x100000001B3ull;
    h = (h ^ H.ref_size) * 0x100000001B3ull;
    h ^= h >> 29;
    h = (h ^ H.query_size) * 0x100000001B3ull;
    h ^= h >> 33;
    h *= 0xFF51AFD7ED558CCDull;
    h ^= h >> 33;
    return h;
  }
  __device__ __forceinline__ bool same(u32 i, u32 j) const {
    const wga_stat_row_head& A = heads[i];
    const wga_stat_row_head& B = heads[j];
    const u32 ra = name_span_len(A.rname_off, A.rname_len, n_name_bytes), qa = name_span_len(A.qname_off, A.qname_len, n_name_bytes);
    const u32 rb = name_span_len(B.rname_off, B.rname_len, n_name_bytes), qb = name_span_len(B.qname_off, B.qname_len, n_name_bytes);
    bool same = ra == rb && qa == qb && A.ref_size == B.ref_size && A.query_size == B.query_size;
    for (u32 k = 0; same && k < ra; k++) same = names[A.rname_off + k] == names[B.rname_off + k];
    for (u32 k = 0; same && k < qa; k++) same = names[A.qname_off + k] == names[B.qname_off + k];
    return same;
  }
};

struct SortStatPairKey { /* the sort's key of a payload: the record's pair */
  const u32* gs;
  __device__ __forceinline__ u32 operator()(u32 i) const { return gs[i]; }
};

/* sorted place p: the pairs' first places (gstart[n_pairs] = n) */
__global__ __launch_bounds__(256) void k_stat_pairs_bounds(u64 n, u64 n_pairs, const u32* __restrict__ order,
                                                           const u32* __restrict__ gs, u32* __restrict__ gstart, K36Hdr* hdr,
                                                           u64 where) {
  const u64 p = (u64)blockIdx.x * 256u + threadIdx.x;
  if (p >= n) return;
  if (p == 0u) {
    hdr->n = n, hdr->n_pairs = n_pairs, hdr->where = where;
    hdr->filled[0] = hdr->filled[1] = 0u;
  }
  const u32 i = order[p] < n ? order[p] : 0u;
  const u32 g = gs[i];
  bool first = true;
  if (p > 0u) first = gs[order[p - 1u] < n ? order[p - 1u] : 0u] != g;
  if (first && (u64)g < n_pairs) gstart[g] = (u32)p;
  if (p + 1u == n) gstart[n_pairs] = (u32)n;
}

struct ScanStatPairInv { /* scan functor: sorted place p holds an inverted record */
  const u32* order;
  const wga_cigar_counts* counts;
  u32 n;
  __device__ u64 operator()(u32 p) const {
    const u32 i = order[p];
    return i < n && counts[i].inv_ev != 0u ? 1u : 0u;
  }
};

/* the inverted records' f32 inv_size values, in sorted order (invsc = the exclusive scan of ScanStatPairInv) */
__global__ __launch_bounds__(256) void k_stat_pairs_inv_vals(u64 n, const u32* __restrict__ order,
                                                             const wga_cigar_counts* __restrict__ counts,
                                                             const u64* __restrict__ invsc, u32* __restrict__ inv_val) {
  const u64 p = (u64)blockIdx.x * 256u + threadIdx.x;
  if (p >= n) return;
  const u32 i = order[p];
  if (i >= n) return;
  const wga_cigar_counts c = counts[i];
  if (c.inv_ev == 0u) return;
  const u64 at = invsc[p];
  if (at < n) inv_val[at] = stat_row_f32(c, c.match + c.mismatch + c.del_bp + c.inv_del_bp).inv_size;
}

__global__ __launch_bounds__(256) void k_stat_pairs_of_rec(u64 n, const u32* __restrict__ gs, u32* __restrict__ pair_of_rec) {
  const u64 i = (u64)blockIdx.x * 256u + threadIdx.x;
  if (i < n) pair_of_rec[i] = gs[i];
}

/* pair g: what does not depend on the sums */
__global__ __launch_bounds__(256) void k_stat_pairs_init(u64 n, u64 n_pairs, const u32* __restrict__ order,
                                                         const u32* __restrict__ gstart,
                                                         const wga_stat_row_head* __restrict__ heads,
                                                         wga_stat_pair_dev* __restrict__ pairs) {
  const u64 g = (u64)blockIdx.x * 256u + threadIdx.x;
  if (g >= n_pairs) return;
  const u32 p = gstart[g] < n ? gstart[g] : 0u;
  const u32 first = order[p] < n ? order[p] : 0u; /* the pair's lowest record: the sort is stable */
  wga_stat_pair_dev P;
  for (u32 k = 0; k < 11u; k++) P.sum[k] = 0u;
  P.inv_size_bits = P.pad = 0u;
  P.first_rec = first;
  P.n_recs = (u64)gstart[g + 1u] - p;
  P.ref_start = heads[first].ref_size; /* the minima start from the sizes */
  P.query_start = heads[first].query_size;
  pairs[g] = P;
}

#define WGA_STAT_PAIR_VALS 13u /* the eleven counters and the two starts */

__global__ __launch_bounds__(256) void k_stat_pairs_reduce(u64 n, u64 n_pairs, const u32* __restrict__ order,
                                                           const u32* __restrict__ gs, const u32* __restrict__ gstart,
                                                           const wga_stat_row_head* __restrict__ heads,
                                                           const wga_cigar_counts* __restrict__ counts,
                                                           wga_stat_pair_dev* __restrict__ pairs) {
  __shared__ u64 s_acc[256][WGA_STAT_PAIR_VALS];
  const u32 tid = threadIdx.x, lane = tid & 63u;
  const u64 x0 = (u64)blockIdx.x * 256u;
  const u64 x1 = x0 + 256u < n ? x0 + 256u : n;
  const u64 p = x0 + tid;
  for (u32 k = 0; k < WGA_STAT_PAIR_VALS; k++) s_acc[tid][k] = k < 11u ? 0ull : ~0ull;
  const u32 i0 = order[x0] < n ? order[x0] : 0u, i1 = order[x1 - 1u] < n ? order[x1 - 1u] : 0u;
  const u32 g0 = gs[i0], g1 = gs[i1]; /* the block's first and last pair */
  __syncthreads();
  const bool live = p < x1;
  u64 v[WGA_STAT_PAIR_VALS];
  u32 slot = 0xFFFFFFFFu;
  if (live) {
    const u32 i = order[p] < n ? order[p] : 0u;
    slot = gs[i] - g0; /* the sorted pairs ascend in steps of one: at most tid */
    const wga_cigar_counts c = counts[i];
    const u64 a[11] = {c.match, c.mismatch, c.ins_ev, c.ins_bp, c.del_ev, c.del_bp, c.inv_ins_ev, c.inv_ins_bp, c.inv_del_ev,
                       c.inv_del_bp, c.inv_ev};
#pragma unroll
    for (u32 k = 0; k < 11u; k++) v[k] = a[k];
    v[11] = heads[i].ref_start;
    v[12] = heads[i].query_start;
  } else {
#pragma unroll
    for (u32 k = 0; k < WGA_STAT_PAIR_VALS; k++) v[k] = k < 11u ? 0ull : ~0ull;
  }
  /* a wave of one pair: its sums by shuffles, one lane adds them */
  const u32 slot_lo = __shfl(slot, 0);
  const bool one_pair = __ballot(live && slot == slot_lo) == ~0ull;
  if (one_pair) {
#pragma unroll
    for (u32 k = 0; k < WGA_STAT_PAIR_VALS; k++)
      for (u32 d = 32u; d; d >>= 1) {
        const u64 o = __shfl_xor(v[k], (int)d);
        v[k] = k < 11u ? v[k] + o : (o < v[k] ? o : v[k]);
      }
  }
  if (live && slot < 256u && (!one_pair || lane == 0u)) {
#pragma unroll
    for (u32 k = 0; k < 11u; k++)
      if (v[k]) atomicAdd(&s_acc[slot][k], v[k]);
    atomicMin(&s_acc[slot][11], v[11]);
    atomicMin(&s_acc[slot][12], v[12]);
  }
  __syncthreads();
  const u64 g = (u64)g0 + tid;
  if (g > (u64)g1 || g >= n_pairs) return;
  const bool inside = (u64)gstart[g] >= x0 && (u64)gstart[g + 1u] <= x1; /* no other block holds a record of this pair */
  wga_stat_pair_dev& P = pairs[g];
  u64* sum = P.sum;
  if (inside) {
    for (u32 k = 0; k < 11u; k++) sum[k] = s_acc[tid][k];
    if (s_acc[tid][11] < P.ref_start) P.ref_start = s_acc[tid][11];
    if (s_acc[tid][12] < P.query_start) P.query_start = s_acc[tid][12];
  } else {
    for (u32 k = 0; k < 11u; k++)
      if (s_acc[tid][k]) atomicAdd(&sum[k], s_acc[tid][k]);
    atomicMin(&P.ref_start, s_acc[tid][11]);
    atomicMin(&P.query_start, s_acc[tid][12]);
  }
}

__device__ __forceinline__ float f32_of_bits(u32 b) {
  float f;
  memcpy(&f, &b, 4);
  return f;
}

/* one wave per pair: inv_size_bits = the left fold, in sorted (= record) order, of the pair's inverted records' values */
__global__ __launch_bounds__(256) void k_stat_pairs_fold(u64 n, u64 n_pairs, const u32* __restrict__ gstart,
                                                         const u64* __restrict__ invsc, const u32* __restrict__ inv_val,
                                                         const u32* __restrict__ inv_in, wga_stat_pair_dev* __restrict__ pairs,
                                                         K36Hdr* hdr, u64 filled0, u64 filled1) {
  const u32 lane = threadIdx.x & 63u;
  const u64 g = (u64)blockIdx.x * 4u + (threadIdx.x >> 6); /* wave-uniform */
  if (blockIdx.x == 0u && threadIdx.x == 0u) hdr->filled[0] = filled0, hdr->filled[1] = filled1; /* the outputs now hold the rest */
  if (g >= n_pairs) return;
  const u32 p0 = gstart[g], p1 = gstart[g + 1u];
  u64 lo = 0, hi = 0;
  if ((u64)p0 <= (u64)p1 && (u64)p1 <= n) lo = invsc[p0], hi = invsc[p1];
  if (lo > hi || hi > n) lo = hi = 0;
  float acc = inv_in ? f32_of_bits(inv_in[g]) : 0.0f;
  for (u64 base = lo; base < hi; base += 64u) {
    const u32 cnt = hi - base < 64u ? (u32)(hi - base) : 64u;
    const float x = lane < cnt ? f32_of_bits(inv_val[base + lane]) : 0.0f;
    for (u32 l = 0; l < cnt; l++) acc += __shfl(x, (int)l); /* lane order: every lane holds the same accumulator */
  }
  if (lane == 0u) pairs[g].inv_size_bits = f32_bits(acc);
}

/* ---- the pairs' rows: a second source for K33's row writer ------------------------------------------------------------------- */
/* Row r is pair r: K33's 22 columns over the pair's sums, with column 8 = ref_size - aligned_size (mod 2^64, stat.rs:216) and
 * column 18 the given f32 */
struct StatPairRowSrc {
  static constexpr u32 kStage = WGA_STAT_ROWS_STAGE;
  const u8* names;
  u64 n_name_bytes;
  const wga_stat_row_head* heads;
  const wga_cigar_counts* counts; /* the sums */
  const u32* inv_bits;
  template <typename S>
  __device__ __forceinline__ void emit(S& s, u32 r) const {
    stat_row_emit<true>(s, heads[r], names, n_name_bytes, counts[r], inv_bits[r]);
  }
};
struct StatPairRowsFmt : RecordRowsFmt<StatPairRowSrc> {};

/* plan[r] = the bytes of row r (k_record_rows_plan's sources have four fields; this one has five) */
__global__ __launch_bounds__(256) void k_stat_pair_rows_plan(StatPairRowSrc src, u32 n, u64* __restrict__ plan) {
  const u64 r = (u64)blockIdx.x * 256u + threadIdx.x;
  if (r >= (u64)n) return;
  TextCount t;
  src.emit(t, (u32)r);
  plan[r] = t.n;
}

#endif /* WGA_K36_STAT_PAIRS_H */
