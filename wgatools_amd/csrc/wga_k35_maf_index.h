/*
 * wga_k35_maf_index.h — K35: `maf-index` on the device (tools/index.rs:14-94): the blocks' file offsets, the name groups and the
 * JSON interval text of every name, from K14's line table of a piece.
 * One header per kernel family; wga_capi.cpp includes them in dependency order (a header may use helpers of the ones in front of it).
 * wga_maf_index, passes of the count call:
 *   newlines  K24's k_paf_newlines: the positions of the newlines in order, which give every line its end (wga_maf_line does not
 *             carry it).
 *   lines     k_maf_index_lines: the lowest WGA_MAF_FALLBACK line (atomicMin) and whether the last line is an s-line; then ONE scan
 *             over the lines of (is an s-line | opens a run << 32): an s-line's rank among the s-lines and its block.
 *   offsets   k_maf_index_offsets: the line behind a run ends it, and the position behind that line's newline is the offset of the
 *             NEXT block (blk_off[blocks in front of the line]); blk_off[0] is the header line's end or the caller's carry.  The
 *             s-lines are listed (sl_line).
 *   groups    K24's table, keyed by the name alone (k_maf_index_init / _claim / _settle): an open-addressing table of 2^k >= 2 n
 *             slots built from atomicMin; the hash only places a name, the bytes decide.  The slot's s-line is the lowest of its
 *             group, so a scan over "is its group's first" numbers the groups by ascending first s-line.  The settle pass also
 *             takes the lowest s-line whose isref differs from its group's first (atomicMin).
 *   sort      wga_sort.h: the s-lines arranged by group number, file order within a group.
 *   items     k_maf_index_items: sorted place p becomes an interval {start, end, offset, strand, first of its group}; a place whose
 *             predecessor has the same group and the same block is a duplicate name in a record (atomicMin); a group's first place
 *             is gstart[g].
 *   scan      the shared scan over ScanItems<MafIdxFmt>: an item's bytes are its emitter's into a TextCount.
 * and of the fill call:
 *   names     k_maf_index_names: the group table.
 *   fill      k_text_items_fill<MafIdxFmt> (wga_text_out.h): 256 consecutive intervals per block, whatever group borders lie inside
 *             them — a file of two names is spread over as many blocks as one of a million.
 */
#ifndef WGA_K35_MAF_INDEX_H
#define WGA_K35_MAF_INDEX_H

#include "wga_k13_splitters.h"
#include "wga_k24_paf_filter.h" /* k_paf_newlines, paf_pair_slot */
#include "wga_sort.h"
#include "wga_text_out.h"

struct K35Hdr {
  u64 first_dup, first_conflict, first_fallback; /* line indices, WGA_NONE when there is none */
  u64 last_is_s;                                 /* the piece's last line is an s-line: its run has no ending line */
  u64 cnt[2];                                    /* the lengths of the two lists of s-lines without a group (as K24PairHdr) */
  u64 pad[2];
};

struct wga_maf_index_name_dev {
  u64 name_off, size, first_line, n_ivls, text_off;
  u32 name_len, isref;
};

/* an interval of the sorted list: what its text is made of */
struct MafIdxIvl {
  u64 start, end, off;
  u32 flags; /* 1: '-' strand, 2: the first of its group (no comma in front) */
  u32 group;
};

__device__ __forceinline__ bool maf_index_is_s(const wga_maf_line_dev* __restrict__ lines, u64 i) {
  return lines[i].status == WGA_MAF_SLINE;
}

struct ScanMafIdxLine { /* scan functor: (is an s-line) | (opens a run) << 32 */
  const wga_maf_line_dev* lines;
  __device__ u64 operator()(u32 i) const {
    if (!maf_index_is_s(lines, i)) return 0u;
    return 1ull | ((i == 0u || !maf_index_is_s(lines, i - 1u)) ? 1ull << 32 : 0ull);
  }
};

__global__ __launch_bounds__(256) void k_maf_index_lines(const wga_maf_line_dev* __restrict__ lines, u64 n_lines, K35Hdr* hdr) {
  const u64 i = (u64)blockIdx.x * 256u + threadIdx.x;
  if (i >= n_lines) return;
  const u32 st = lines[i].status;
  if (st == WGA_MAF_FALLBACK) atomicMin(&hdr->first_fallback, i);
  if (i + 1u == n_lines) hdr->last_is_s = st == WGA_MAF_SLINE ? 1u : 0u;
}

/* P = the exclusive scan of ScanMafIdxLine (P[n_lines] = the totals) */
__global__ __launch_bounds__(256) void k_maf_index_offsets(const wga_maf_line_dev* __restrict__ lines, u64 n_lines, u64 n_bytes,
                                                           const u64* __restrict__ n_newlines_p, const u32* __restrict__ nl_pos,
                                                           const u64* __restrict__ P, u64 skip, u64 base, u64 carry,
                                                           u64* __restrict__ blk_off, u32* __restrict__ sl_line) {
  const u64 i = (u64)blockIdx.x * 256u + threadIdx.x;
  if (i >= n_lines) return;
  const u64 end = i < *n_newlines_p ? (u64)nl_pos[i] + 1u : n_bytes; /* behind the line's newline */
  const bool s = maf_index_is_s(lines, i);
  if (i == 0u) blk_off[0] = skip == 0u ? base + end : carry; /* the file's first line is the header, whatever it starts with */
  if (s) sl_line[P[i] & 0xFFFFFFFFull] = (u32)i;
  else if (i > 0u && maf_index_is_s(lines, i - 1u)) blk_off[P[i] >> 32] = base + end - skip;
}

/* FNV-1a over the name and a finaliser, so that the low bits (which pick the slot) depend on every byte */
__device__ __forceinline__ u64 maf_index_hash(const u8* __restrict__ text, const wga_maf_line_dev& L) {
  u64 h = 0xCBF29CE484222325ull;
  for (u32 k = 0; k < L.name_len; k++) h = (h ^ text[L.name_off + k]) * 0x100000001B3ull;
  h ^= h >> 33;
  h *= 0xFF51AFD7ED558CCDull;
  h ^= h >> 33;
  return h;
}

/* every s-line k: its start slot, no group yet, a place in list 0 */
__global__ __launch_bounds__(256) void k_maf_index_init(const u8* __restrict__ text, const wga_maf_line_dev* __restrict__ lines,
                                                        const u32* __restrict__ sl_line, u64 n_s, u64 hash_mask, u32 slot_mask,
                                                        u32* __restrict__ start, u32* __restrict__ rep, u32* __restrict__ list) {
  const u64 k = (u64)blockIdx.x * 256u + threadIdx.x;
  if (k >= n_s) return;
  rep[k] = 0xFFFFFFFFu;
  start[k] = (u32)(maf_index_hash(text, lines[sl_line[k]]) & hash_mask) & slot_mask;
  list[k] = (u32)k;
}

__global__ __launch_bounds__(256) void k_maf_index_claim(const u32* __restrict__ list, u64 m, u64 r, u32 slot_mask,
                                                         const u32* __restrict__ start, u64* __restrict__ slots, K35Hdr* hdr) {
  const u64 x = (u64)blockIdx.x * 256u + threadIdx.x;
  if (x == 0u) hdr->cnt[(r + 1u) & 1u] = 0u; /* the list this round's settle pass appends to */
  if (x >= m) return;
  const u32 k = list[x];
  atomicMin(&slots[paf_pair_slot(start[k], r, slot_mask)], (r << 32) | (u64)k);
}

__global__ __launch_bounds__(256) void k_maf_index_settle(const u8* __restrict__ text, const wga_maf_line_dev* __restrict__ lines,
                                                          const u32* __restrict__ sl_line, const u32* __restrict__ list, u64 m,
                                                          u64 r, u32 slot_mask, const u32* __restrict__ start,
                                                          const u64* __restrict__ slots, u32* __restrict__ rep,
                                                          u32* __restrict__ next, K35Hdr* hdr) {
  const u64 x = (u64)blockIdx.x * 256u + threadIdx.x;
  if (x >= m) return;
  const u32 k = list[x];
  const u32 w = (u32)slots[paf_pair_slot(start[k], r, slot_mask)];
  const u32 ia = sl_line[k], ib = sl_line[w];
  const wga_maf_line_dev& A = lines[ia];
  const wga_maf_line_dev& B = lines[ib];
  bool same = A.name_len == B.name_len; /* the names decide, never the hash */
  for (u32 j = 0; same && j < A.name_len; j++) same = text[A.name_off + j] == text[B.name_off + j];
  if (same) {
    rep[k] = w;
    /* isref = the first line of its run (index.rs:44-58) */
    const bool ra = ia == 0u || !maf_index_is_s(lines, ia - 1u), rb = ib == 0u || !maf_index_is_s(lines, ib - 1u);
    if (ra != rb) atomicMin(&hdr->first_conflict, (u64)ia);
  } else {
    next[atomicAdd(&hdr->cnt[(r + 1u) & 1u], (u64)1)] = k;
  }
}

struct ScanMafIdxRep { /* scan functor: s-line k is its group's first */
  const u32* rep;
  __device__ u64 operator()(u32 k) const { return rep[k] == k ? 1u : 0u; }
};

/* gs[k] = the group of s-line k (gidx = the exclusive scan of ScanMafIdxRep), order[k] = k */
__global__ __launch_bounds__(256) void k_maf_index_groups(u64 n_s, const u32* __restrict__ rep, const u64* __restrict__ gidx,
                                                          u32* __restrict__ gs, u32* __restrict__ order) {
  const u64 k = (u64)blockIdx.x * 256u + threadIdx.x;
  if (k >= n_s) return;
  const u32 w = rep[k];
  gs[k] = w < n_s ? (u32)gidx[w] : 0u;
  order[k] = (u32)k;
}

struct SortMafIdxKey { /* the sort's key of a payload: the s-line's group */
  const u32* gs;
  __device__ __forceinline__ u32 operator()(u32 k) const { return gs[k]; }
};

/* sorted place p: its interval, the duplicate check, the groups' first places (gstart[n_groups] = n_s) */
__global__ __launch_bounds__(256) void k_maf_index_items(const wga_maf_line_dev* __restrict__ lines, const u32* __restrict__ sl_line,
                                                         u64 n_s, u64 n_groups, const u32* __restrict__ order,
                                                         const u32* __restrict__ gs, const u64* __restrict__ P,
                                                         const u64* __restrict__ blk_off, MafIdxIvl* __restrict__ ivl,
                                                         u32* __restrict__ gstart, K35Hdr* hdr, u64 where) {
  const u64 p = (u64)blockIdx.x * 256u + threadIdx.x;
  if (p >= n_s) return;
  if (p == 0u) hdr->pad[0] = where; /* which of the sort's two buffers `order` is: the fill call's names pass reads it there */
  const u32 k = order[p], g = gs[k], i = sl_line[k];
  const u64 blk = (P[i + 1u] >> 32) - 1u; /* the runs opened up to and with line i */
  bool first = true;
  if (p > 0u) {
    const u32 kp = order[p - 1u];
    first = gs[kp] != g;
    if (!first && (P[sl_line[kp] + 1u] >> 32) - 1u == blk) atomicMin(&hdr->first_dup, (u64)i);
  }
  if (first && (u64)g < n_groups) gstart[g] = (u32)p;
  if (p + 1u == n_s) gstart[n_groups] = (u32)n_s;
  const wga_maf_line_dev& L = lines[i];
  MafIdxIvl v;
  v.start = L.num[0];
  v.end = L.num[0] + L.num[1]; /* wraps, as the release build's sum does */
  v.off = blk_off[blk];
  v.flags = (L.strand_neg ? 1u : 0u) | (first ? 2u : 0u);
  v.group = g;
  ivl[p] = v;
}

/* the letters of a word, one c() each: immediates in the fill, a constant in the count */
template <typename S, u32 N>
__device__ __forceinline__ void text_word(S& s, const char (&w)[N]) {
#pragma unroll
  for (u32 k = 0; k + 1u < N; k++) s.c((u8)w[k]);
}

/* [,]{"start":S,"end":E,"strand":"+","offset":O} */
template <typename S>
__device__ __forceinline__ void maf_index_ivl_emit(S& s, const MafIdxIvl& v) {
  if (!(v.flags & 2u)) s.c((u8)',');
  text_word(s, "{\"start\":");
  s.dec(v.start);
  text_word(s, ",\"end\":");
  s.dec(v.end);
  text_word(s, ",\"strand\":\"");
  s.c((v.flags & 1u) ? (u8)'-' : (u8)'+');
  text_word(s, "\",\"offset\":");
  s.dec(v.off);
  s.c((u8)'}');
}

/* the stage: 256 intervals of three 10-digit numbers (1 + 40 + 30 + 1 bytes and the comma); a stretch of longer numbers is
 * written directly */
#define WGA_MAF_INDEX_STAGE (WGA_TEXT_ITEMS * 72u)

struct MafIdxFmt { /* the format of the interval text (wga_text_out.h: an item stream; the records are not looked at) */
  static constexpr u32 kStage = WGA_MAF_INDEX_STAGE;
  static constexpr bool kCheckSize = true;
  const MafIdxIvl* ivl;
  u32 n_rec;
  __device__ __forceinline__ u32 rec(u64, u32, u32) const { return 0u; }
  template <typename S>
  __device__ __forceinline__ void emit(S& s, u64 x, u32) const {
    maf_index_ivl_emit(s, ivl[x]);
  }
  __device__ __forceinline__ u64 size(u64 x, u32) const {
    TextCount c;
    maf_index_ivl_emit(c, ivl[x]);
    return c.n;
  }
};

/* the group table: one entry per group and the closing one (text_off = the text's length, the rest zero) */
__global__ __launch_bounds__(256) void k_maf_index_names(const wga_maf_line_dev* __restrict__ lines, const u32* __restrict__ sl_line,
                                                         u64 n_s, u64 n_groups, const u32* __restrict__ order0,
                                                         const u32* __restrict__ order1, const K35Hdr* __restrict__ hdr,
                                                         const u32* __restrict__ gstart, const u64* __restrict__ isc,
                                                         wga_maf_index_name_dev* __restrict__ names) {
  const u64 g = (u64)blockIdx.x * 256u + threadIdx.x;
  if (g > n_groups) return;
  const u32* __restrict__ order = hdr->pad[0] ? order1 : order0;
  wga_maf_index_name_dev N;
  N.name_off = N.size = N.first_line = N.n_ivls = 0u;
  N.name_len = N.isref = 0u;
  N.text_off = isc[n_s];
  if (g < n_groups) {
    const u32 p = gstart[g] < n_s ? gstart[g] : 0u;
    const u32 i = sl_line[order[p] < n_s ? order[p] : 0u]; /* the group's first s-line: the sort is stable */
    const wga_maf_line_dev& L = lines[i];
    N.name_off = L.name_off;
    N.name_len = L.name_len;
    N.size = L.num[2];
    N.first_line = i;
    N.isref = (i == 0u || !maf_index_is_s(lines, i - 1u)) ? 1u : 0u;
    N.n_ivls = (u64)gstart[g + 1u] - p;
    N.text_off = isc[p];
  }
  names[g] = N;
}

#endif /* WGA_K35_MAF_INDEX_H */
