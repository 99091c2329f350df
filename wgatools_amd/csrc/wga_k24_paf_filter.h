/*
 * wga_k24_paf_filter.h — K24: `filter -f paf` on the device (tools/filter.rs:88-160 with the csv writer of paf.rs:50-65).
 * For a plain line (K13's WGA_PAF_OK) the reference's writer reproduces the line's bytes whenever its nine numbers are in
 * canonical decimal: names and tags pass through unquoted (a line with a quote or a CR is WGA_PAF_FALLBACK), only the numbers
 * are printed anew.  So the filter is a predicate over K13's line table plus an order-preserving compaction of whole lines,
 * and `-a` adds an exact group-by over (query name, target name).
 * wga_paf_filter, passes:
 *   newlines  k_paf_newlines over 4 KiB of text per block with 16-byte loads (count, scan, fill, as k_paf_delims): the positions
 *             of the newlines in order, which give every line its extent (wga_paf_line does not carry it); the fill pass also
 *             knows every byte's line and takes the first line with a byte >= 0x80 by atomicMin.
 *   lines     one thread per line: the keep flag (thresholds, or the pair's flag), the canonical-number check (reads up to the
 *             line's 12th tab: WGA_PAF_NUMBERS_INEXACT, which K29's plan expands too) and the length of the line's text; one scan of (length | keep << 32) places the kept lines
 *             among the kept lines and in the text, k_paf_filter_compact lists them.
 *   fill      the text in tiles of WGA_PAF_FILTER_TILE bytes, one per block: the tile's lines by binary search in the kept
 *             lines' places, their bytes through maf_tile_slices (16-byte groups: one unaligned load + one aligned LDS store
 *             inside a line, bytes at line ends), the tile out in 16-byte stores.  A line of megabytes is spread over its
 *             tiles like any other text.
 * wga_paf_pairs: an open-addressing table of 2^k >= 2 n slots built from atomicMin and atomicAdd alone.  Every OK line hashes
 * its two names to a start slot (the hash only PLACES a pair); in round r every line still without a pair offers
 * (r << 32 | line) to slot start + r (r + 1) / 2 by atomicMin (k_paf_pairs_claim: a slot taken in an earlier round keeps its
 * smaller value), then compares its names byte for byte with the slot's line (k_paf_pairs_settle): equal names — the line
 * joins that pair, whose representative is the slot's line; otherwise it goes to the next round.  The lines of a pair hash
 * alike and move in lockstep, so the slot's line is the pair's lowest line.  Sums are atomicAdd on the representative's
 * entry (u64, wrapping); a scan over "is a representative" numbers the pairs by ascending first line.
 */
#ifndef WGA_K24_PAF_FILTER_H
#define WGA_K24_PAF_FILTER_H

#include "wga_k13_splitters.h"
#include "wga_maf_write.h" /* maf_find, maf_tile_slices, lds_text_flush */

#define WGA_PAF_FILTER_TILE WGA_MAF_TILE /* bytes of text per fill block */
/* lines one tile can meet: the shortest OK line, twelve fields of which nine hold a digit and one the strand, is 21 bytes and its
 * newline, so ceil(8192 / 22) + 1 = 374 */
#define WGA_PAF_FILTER_TILE_LINES 384u

struct K24Hdr {
  u64 first_inexact; /* the lowest inexact line, WGA_NONE when there is none */
  u64 pad;
};

struct wga_paf_filter_params_dev {
  u64 min_block_size, min_query_size;
  const u32* pair_of_line;
  const u8* pair_keep;
};

/* the newlines of 4 KiB of text per block.  FILL: their positions at nl_pos[rank] (only ranks below cap: the caller's n_lines
 * bounds the list), and the line of the first byte >= 0x80 (a byte's line is the number of newlines in front of it) */
template <bool FILL>
__global__ __launch_bounds__(256) void k_paf_newlines(const u8* __restrict__ text, u64 n_bytes, u64* blk, const u64* blk_off,
                                                      u32* __restrict__ nl_pos, u64 cap, K24Hdr* hdr) {
  __shared__ u64 s_w[5];
  const u64 c = ((u64)blockIdx.x * 256u + threadIdx.x) * 16u;
  u32 w[4] = {0, 0, 0, 0};
  if (c + 16u <= n_bytes) {
    const u32x4_a1 a = *(const u32x4_a1*)(text + c);
    w[0] = a[0], w[1] = a[1], w[2] = a[2], w[3] = a[3];
  } else if (c < n_bytes) {
    for (u32 j = 0; j < (u32)(n_bytes - c); j++) w[j >> 2] |= (u32)text[c + j] << (8u * (j & 3u));
  }
  u32 nm = 0, hm = 0;
#pragma unroll
  for (int d = 0; d < 4; d++) {
#pragma unroll
    for (int b = 0; b < 4; b++) {
      const u32 ch = (w[d] >> (8 * b)) & 0xFFu;
      const u32 bit = 1u << (4 * d + b);
      nm |= ch == 0x0Au ? bit : 0u;
      hm |= ch >= 0x80u ? bit : 0u;
    }
  }
  u64 tot;
  const u64 ex = block_excl_scan_u64((u64)__builtin_popcount(nm), s_w, &tot);
  if (!FILL) {
    if (threadIdx.x == 0) blk[blockIdx.x] = tot;
    return;
  }
  u64 ni = blk_off[blockIdx.x] + ex;
  if (hm) atomicMin(&hdr->first_inexact, ni + (u64)__builtin_popcount(nm & ((1u << __builtin_ctz(hm)) - 1u)));
  while (nm) {
    const u32 j = (u32)__builtin_ctz(nm);
    nm &= nm - 1u;
    if (ni < cap) nl_pos[ni] = (u32)(c + j);
    ni++;
  }
}

/* line i = text[s, e): behind the newline in front of it, up to its own newline or the text's end */
__device__ __forceinline__ void paf_line_extent(const u32* __restrict__ nl_pos, u64 n_newlines, u64 n_bytes, u64 i, u64* s,
                                                u64* e) {
  *s = i ? (u64)nl_pos[i - 1] + 1u : 0u;
  *e = i < n_newlines ? (u64)nl_pos[i] : n_bytes;
}

/* the exactness predicate's part on an OK line text[s, e), shared by K24's filter and K29's plan: the csv writer prints the nine
 * numbers anew (u64 Display), so `+5`, `007` and `00` would change.  Sets `inexact`, never clears it.  A macro and not a function:
 * k_paf_filter_lines keeps, instruction for instruction, the code it had when the loop stood in it. */
#define WGA_PAF_NUMBERS_INEXACT(text, s, e, inexact)                                               \
  {                                                                                                \
    u64 fs = (s);                                                                                  \
    for (u32 nf = 0; nf < 12u && fs <= (e); nf++) {                                                \
      if (nf - 1u < 3u || nf - 6u < 6u) {                                                          \
        const u32 c0 = fs < (e) ? (text)[fs] : 0u, c1 = fs + 1u < (e) ? (text)[fs + 1u] : 0u;      \
        if (c0 == (u32)'+' || (c0 == (u32)'0' && c1 - 0x30u <= 9u)) (inexact) = true;              \
      }                                                                                            \
      while (fs < (e) && (text)[fs] != 0x09u) fs++;                                                \
      fs++;                                                                                        \
    }                                                                                              \
  }

/* val[i] = the bytes line i adds to the text (its own and a newline; 0 when it is dropped) | kept << 32 */
__global__ __launch_bounds__(256) void k_paf_filter_lines(const u8* __restrict__ text, u64 n_bytes, u64 n_lines,
                                                          const u64* __restrict__ n_newlines_p,
                                                          const u32* __restrict__ nl_pos,
                                                          const wga_paf_line_dev* __restrict__ lines,
                                                          wga_paf_filter_params_dev P, u64* __restrict__ val, K24Hdr* hdr) {
  const u64 i = (u64)blockIdx.x * 256u + threadIdx.x;
  if (i >= n_lines) return;
  u64 s, e;
  paf_line_extent(nl_pos, *n_newlines_p, n_bytes, i, &s, &e);
  if (e < s) e = s; /* a line table that is not this text's: nothing is read outside the text */
  const u32 status = lines[i].status;
  bool inexact = status == WGA_PAF_FALLBACK, keep = false;
  if (status == WGA_PAF_OK) {
    WGA_PAF_NUMBERS_INEXACT(text, s, e, inexact)
    if (P.pair_keep) {
      const u32 p = P.pair_of_line[i];
      keep = p != 0xFFFFFFFFu && P.pair_keep[p] != 0;
    } else { /* filter.rs:96-101: both compare with `<`, the span wraps */
      keep = !(lines[i].num[5] - lines[i].num[4] < P.min_block_size || lines[i].num[0] < P.min_query_size);
    }
  }
  if (inexact) atomicMin(&hdr->first_inexact, i);
  val[i] = keep ? (e - s + 1u) | (1ull << 32) : 0u;
}

/* the kept lines in order: koff[k] = the k-th kept line's place in the text (koff[n_kept] = the text's length), ksrc[k] = where
 * its bytes start.  P = the exclusive scan of val (P[n_lines] = the totals) */
__global__ __launch_bounds__(256) void k_paf_filter_compact(u64 n_lines, const u32* __restrict__ nl_pos,
                                                            const u64* __restrict__ P, u64* __restrict__ koff,
                                                            u64* __restrict__ ksrc) {
  const u64 i = (u64)blockIdx.x * 256u + threadIdx.x;
  if (i >= n_lines) return;
  const u64 a = P[i], b = P[i + 1u];
  if ((a >> 32) != (b >> 32)) {
    koff[a >> 32] = a & 0xFFFFFFFFull;
    ksrc[a >> 32] = i ? (u64)nl_pos[i - 1] + 1u : 0u;
  }
  if (i + 1u == n_lines) koff[b >> 32] = b & 0xFFFFFFFFull;
}

/* one tile of the text (blockIdx.x, 256 threads): the kept lines [0, nk), `total` bytes in all */
__global__ __launch_bounds__(256) void k_paf_filter_fill(const u8* __restrict__ text, const u64* __restrict__ koff,
                                                         const u64* __restrict__ ksrc, u32 nk, u64 total,
                                                         u8* __restrict__ out) {
  __shared__ u32x4_a16 s_tile[WGA_PAF_FILTER_TILE / 16u];
  __shared__ u32 s_lo[WGA_PAF_FILTER_TILE_LINES], s_hi[WGA_PAF_FILTER_TILE_LINES];
  __shared__ u64 s_src[WGA_PAF_FILTER_TILE_LINES];
  __shared__ u32 s_first, s_count;
  u8* const tbuf = (u8*)s_tile;
  const u32 tid = threadIdx.x;
  const u64 T0 = (u64)blockIdx.x * WGA_PAF_FILTER_TILE;
  const u32 tl = (u32)(total - T0 < WGA_PAF_FILTER_TILE ? total - T0 : WGA_PAF_FILTER_TILE);
  if (tid == 0u) {
    const u32 l0 = maf_find(koff, nk, T0);
    const u32 lim = nk - l0 < WGA_PAF_FILTER_TILE_LINES ? nk : l0 + WGA_PAF_FILTER_TILE_LINES;
    s_first = l0;
    s_count = maf_find_in(koff, l0, lim, T0 + tl - 1u) - l0 + 1u;
  }
  __syncthreads();
  const u32 l0 = s_first, nl = s_count; /* nl <= WGA_PAF_FILTER_TILE_LINES */
  for (u32 j = tid; j < nl; j += 256u) {
    /* the line's bytes are [a, z) of the tile, its newline is at z: both clipped to the tile */
    const long long a = (long long)(koff[l0 + j] - T0), z = (long long)(koff[l0 + j + 1u] - T0) - 1;
    const long long lo = a < 0 ? 0 : a, hi = z > (long long)tl ? (long long)tl : z;
    s_lo[j] = (u32)lo;
    s_hi[j] = (u32)(hi < lo ? lo : hi);
    s_src[j] = ksrc[l0 + j] + (u64)(lo - a);
    if (z >= 0 && z < (long long)tl) tbuf[z] = 0x0Au;
  }
  __syncthreads();
  maf_tile_slices(tbuf, tl, nl, s_lo, s_hi, s_src, text, tid);
  __syncthreads();
  lds_text_flush(tbuf, 0u, tl, out + T0, tid, 256u);
}

/* ---- pairs ----------------------------------------------------------------------------------------------------------------- */
struct wga_paf_pair_dev {
  u64 first_line, sum, qname_off, tname_off;
  u32 qname_len, tname_len;
};
struct K24PairHdr {
  u64 cnt[2]; /* the lengths of the two lists of lines without a pair: round r reads list r & 1 and appends to the other */
};
#define WGA_PAF_PAIR_EMPTY 0xFFFFFFFFFFFFFFFFull

/* FNV-1a over the query name, a byte no name's end can be mistaken for, the target name; then a finaliser, so that the low
 * bits (which pick the slot) depend on every byte */
__device__ __forceinline__ u64 paf_pair_hash(const u8* __restrict__ text, const wga_paf_line_dev& L) {
  u64 h = 0xCBF29CE484222325ull;
  for (u32 k = 0; k < L.qname_len; k++) h = (h ^ text[L.qname_off + k]) * 0x100000001B3ull;
  h = (h ^ 0xFFull) * 0x100000001B3ull;
  h = (h ^ (u64)L.qname_len) * 0x100000001B3ull;
  for (u32 k = 0; k < L.tname_len; k++) h = (h ^ text[L.tname_off + k]) * 0x100000001B3ull;
  h ^= h >> 33;
  h *= 0xFF51AFD7ED558CCDull;
  h ^= h >> 33;
  return h;
}

/* every OK line: its start slot, no pair yet, a place in list 0 */
__global__ __launch_bounds__(256) void k_paf_pairs_init(const u8* __restrict__ text, const wga_paf_line_dev* __restrict__ lines,
                                                        u64 n_lines, u64 hash_mask, u32 slot_mask, u32* __restrict__ start,
                                                        u32* __restrict__ rep, u64* __restrict__ sum, u32* __restrict__ list,
                                                        K24PairHdr* hdr) {
  const u64 i = (u64)blockIdx.x * 256u + threadIdx.x;
  if (i >= n_lines) return;
  rep[i] = 0xFFFFFFFFu;
  sum[i] = 0u;
  if (lines[i].status != WGA_PAF_OK) return;
  start[i] = (u32)(paf_pair_hash(text, lines[i]) & hash_mask) & slot_mask;
  list[atomicAdd(&hdr->cnt[0], (u64)1)] = (u32)i;
}

__device__ __forceinline__ u32 paf_pair_slot(u32 start, u64 r, u32 slot_mask) {
  return (u32)((u64)start + ((r * (r + 1u)) >> 1)) & slot_mask; /* triangular probing: every slot of a 2^k table */
}

__global__ __launch_bounds__(256) void k_paf_pairs_claim(const u32* __restrict__ list, u64 m, u64 r, u32 slot_mask,
                                                         const u32* __restrict__ start, u64* __restrict__ slots, K24PairHdr* hdr) {
  const u64 x = (u64)blockIdx.x * 256u + threadIdx.x;
  if (x == 0u) hdr->cnt[(r + 1u) & 1u] = 0u; /* the list this round's settle pass appends to */
  if (x >= m) return;
  const u32 i = list[x];
  atomicMin(&slots[paf_pair_slot(start[i], r, slot_mask)], (r << 32) | (u64)i);
}

__global__ __launch_bounds__(256) void k_paf_pairs_settle(const u8* __restrict__ text,
                                                          const wga_paf_line_dev* __restrict__ lines,
                                                          const u32* __restrict__ list, u64 m, u64 r, u32 slot_mask,
                                                          const u32* __restrict__ start, const u64* __restrict__ slots,
                                                          u32* __restrict__ rep, u64* __restrict__ sum, u32* __restrict__ next,
                                                          K24PairHdr* hdr) {
  const u64 x = (u64)blockIdx.x * 256u + threadIdx.x;
  if (x >= m) return;
  const u32 i = list[x];
  const u32 w = (u32)slots[paf_pair_slot(start[i], r, slot_mask)];
  const wga_paf_line_dev& A = lines[i];
  const wga_paf_line_dev& B = lines[w];
  bool same = A.qname_len == B.qname_len && A.tname_len == B.tname_len; /* the names decide, never the hash */
  for (u32 k = 0; same && k < A.qname_len; k++) same = text[A.qname_off + k] == text[B.qname_off + k];
  for (u32 k = 0; same && k < A.tname_len; k++) same = text[A.tname_off + k] == text[B.tname_off + k];
  if (same) {
    rep[i] = w;
    atomicAdd(&sum[w], A.num[5] - A.num[4]); /* wraps, as the release build's sum does */
  } else {
    next[atomicAdd(&hdr->cnt[(r + 1u) & 1u], (u64)1)] = i;
  }
}

struct ScanPairRep {
  const u32* rep;
  __device__ u64 operator()(u32 i) const { return rep[i] == i ? 1u : 0u; }
};

__global__ __launch_bounds__(256) void k_paf_pairs_emit(const wga_paf_line_dev* __restrict__ lines, u64 n_lines,
                                                        const u32* __restrict__ rep, const u64* __restrict__ sum,
                                                        const u64* __restrict__ pidx, u32* __restrict__ pair_of_line,
                                                        wga_paf_pair_dev* __restrict__ pairs) {
  const u64 i = (u64)blockIdx.x * 256u + threadIdx.x;
  if (i >= n_lines) return;
  const u32 w = rep[i];
  pair_of_line[i] = w == 0xFFFFFFFFu ? 0xFFFFFFFFu : (u32)pidx[w];
  if (w != (u32)i) return;
  wga_paf_pair_dev p;
  p.first_line = i;
  p.sum = sum[i];
  p.qname_off = lines[i].qname_off;
  p.tname_off = lines[i].tname_off;
  p.qname_len = lines[i].qname_len;
  p.tname_len = lines[i].tname_len;
  pairs[pidx[i]] = p;
}

#endif /* WGA_K24_PAF_FILTER_H */
