/*
 * wga_k29_paf_fix.h — K29: `validate --fix` on the device (tools/validate.rs:71-141 with the csv writer of paf.rs:50-65).
 * K24's observation holds here: for a plain line whose nine numbers are in canonical decimal the csv writer gives back the line's
 * own bytes, and `--fix` changes at most two of those numbers per record, column 4 (query_end) and column 9 (target_end).  So the
 * fixed file is the input with up to two decimal fields per line printed anew, and the report's two lists name the few records
 * that were wrong.
 * wga_paf_fix_plan, passes:
 *   newlines  K24's k_paf_newlines: every line's extent, and the first line with a byte >= 0x80.
 *   lines     one thread per line: UNTAKEN (K24's exactness predicate, or an OK line without a cg:Z: span) by atomicMin, and
 *             the OK flag whose scan numbers the records; the second call copies the cg spans to the records' places.
 * wga_paf_fix, passes:
 *   newlines  as above (the call keeps nothing of the plan's).
 *   records   a scan of the OK flags, then one thread per line: the two ends from the record's counts, the spans of columns 4
 *             and 9 by the line's first nine tabs, all of it into the record's K29Rec; scans over the records give the rows'
 *             places, the two lists' places and the two counts of bad ends.
 *   fill      the rows in tiles of WGA_PAF_FIX_TILE bytes, one per block, as K24's fill: the tile's records by binary search
 *             in the rows' places; a row is copy, number, copy, number, copy and its newline — the numbers and the newline go
 *             into the LDS image by their record's thread, the (up to three) copies through maf_tile_slices in 16-byte groups,
 *             the tile out in 16-byte stores.  A column that keeps its value is part of the copy around it.
 *   lists     one thread per record with a bad end: `<name>:<start>-<old end>\n` at its scanned place.
 */
#ifndef WGA_K29_PAF_FIX_H
#define WGA_K29_PAF_FIX_H

#include "wga_k24_paf_filter.h" /* k_paf_newlines, paf_line_extent, WGA_PAF_NUMBERS_INEXACT, K24Hdr */

#define WGA_PAF_FIX_TILE WGA_MAF_TILE /* bytes of rows per fill block */
/* records one tile can meet: a row is no shorter than the shortest OK line (WGA_PAF_FILTER_TILE_LINES), a fixed end has a digit */
#define WGA_PAF_FIX_TILE_LINES WGA_PAF_FILTER_TILE_LINES
#define WGA_PAF_FIX_QBAD 1u
#define WGA_PAF_FIX_TBAD 2u

struct K29Rec {
  u64 src;                /* the line's first byte */
  u64 eq, et;             /* the ends the counts give */
  u32 len;                /* the line's bytes, its newline not among them */
  u32 f4b, f4e, f9b, f9e; /* columns 4 and 9 as [b, e) of the line; a column that stays is empty: f4 at 0, f9 at len */
  u32 flags;              /* WGA_PAF_FIX_QBAD | WGA_PAF_FIX_TBAD */
  u32 line;               /* the record's line */
  u32 pad;
};

/* ---- plan -------------------------------------------------------------------------------------------------------------------- */
/* val[i] = line i is a record; hdr->first_inexact takes the lowest untaken line */
__global__ __launch_bounds__(256) void k_paf_fix_plan_lines(const u8* __restrict__ text, u64 n_bytes, u64 n_lines,
                                                            const u64* __restrict__ n_newlines_p,
                                                            const u32* __restrict__ nl_pos,
                                                            const wga_paf_line_dev* __restrict__ lines, u64* __restrict__ val,
                                                            K24Hdr* hdr) {
  const u64 i = (u64)blockIdx.x * 256u + threadIdx.x;
  if (i >= n_lines) return;
  u64 s, e;
  paf_line_extent(nl_pos, *n_newlines_p, n_bytes, i, &s, &e);
  if (e < s) e = s; /* a line table that is not this text's: nothing is read outside the text */
  const u32 status = lines[i].status;
  bool untaken = status == WGA_PAF_FALLBACK;
  if (status == WGA_PAF_OK) {
    WGA_PAF_NUMBERS_INEXACT(text, s, e, untaken)
    if (lines[i].cg_beg == WGA_NONE) untaken = true; /* the reference unwraps an error there: the host path's text */
  }
  if (untaken) atomicMin(&hdr->first_inexact, i);
  val[i] = status == WGA_PAF_OK ? 1u : 0u;
}

/* P = the exclusive scan of the OK flags: record P[i] is line i */
__global__ __launch_bounds__(256) void k_paf_fix_plan_spans(u64 n_lines, const wga_paf_line_dev* __restrict__ lines,
                                                            const u64* __restrict__ P, u64* __restrict__ cg_beg,
                                                            u64* __restrict__ cg_end) {
  const u64 i = (u64)blockIdx.x * 256u + threadIdx.x;
  if (i >= n_lines) return;
  const u64 k = P[i];
  if (k == P[i + 1u]) return;
  cg_beg[k] = lines[i].cg_beg;
  cg_end[k] = lines[i].cg_end;
}

/* ---- fix: records ------------------------------------------------------------------------------------------------------------ */
struct ScanPafOk {
  const wga_paf_line_dev* lines;
  __device__ u64 operator()(u32 i) const { return lines[i].status == WGA_PAF_OK ? 1u : 0u; }
};

__global__ __launch_bounds__(256) void k_paf_fix_lines(const u8* __restrict__ text, u64 n_bytes, u64 n_lines,
                                                       const u64* __restrict__ n_newlines_p, const u32* __restrict__ nl_pos,
                                                       const wga_paf_line_dev* __restrict__ lines, const u64* __restrict__ R,
                                                       const wga_cigar_counts* __restrict__ counts,
                                                       K29Rec* __restrict__ recs) {
  const u64 i = (u64)blockIdx.x * 256u + threadIdx.x;
  if (i >= n_lines) return;
  const u64 k = R[i];
  if (k == R[i + 1u]) return; /* not a record */
  u64 s, e;
  paf_line_extent(nl_pos, *n_newlines_p, n_bytes, i, &s, &e);
  if (e < s) e = s;
  const wga_paf_line_dev& L = lines[i];
  const wga_cigar_counts& c = counts[k];
  K29Rec r;
  r.src = s;
  r.len = (u32)(e - s);
  r.line = (u32)i;
  r.pad = 0u;
  /* validate.rs:82-100: u64 sums, wrapping as the release build's */
  const u64 mx = c.match + c.mismatch;
  r.eq = L.num[1] + mx + c.ins_bp + c.inv_ins_bp;
  r.et = L.num[4] + mx + c.del_bp + c.inv_del_bp;
  /* columns 4 and 9 by the tabs from the line's first byte (a taken line has no tab inside a name) */
  u32 tabs = 0, f4b = 0, f4e = 0, f9b = 0, f9e = 0;
  for (u64 p = s; p < e && tabs < 9u; p++) {
    if (text[p] != 0x09u) continue;
    tabs++;
    const u32 at = (u32)(p - s);
    if (tabs == 3u) f4b = at + 1u;
    if (tabs == 4u) f4e = at;
    if (tabs == 8u) f9b = at + 1u;
    if (tabs == 9u) f9e = at;
  }
  const bool found = tabs == 9u; /* otherwise the table is not this text's: the line is copied as it is */
  const bool qbad = found && r.eq != L.num[2], tbad = found && r.et != L.num[5];
  r.flags = (qbad ? WGA_PAF_FIX_QBAD : 0u) | (tbad ? WGA_PAF_FIX_TBAD : 0u);
  r.f4b = qbad ? f4b : 0u;
  r.f4e = qbad ? f4e : 0u;
  r.f9b = tbad ? f9b : r.len;
  r.f9e = tbad ? f9e : r.len;
  recs[k] = r;
}

/* the bytes of record k's row: the line and its newline, a bad end's digits in place of the column's */
__device__ __forceinline__ u64 paf_fix_row_len(const K29Rec& r) {
  u64 n = (u64)r.len + 1u;
  if (r.flags & WGA_PAF_FIX_QBAD) n = n - (r.f4e - r.f4b) + dec_digits(r.eq);
  if (r.flags & WGA_PAF_FIX_TBAD) n = n - (r.f9e - r.f9b) + dec_digits(r.et);
  return n;
}
/* `<name>:<start>-<end>\n` */
__device__ __forceinline__ u64 paf_fix_item_len(u32 name_len, u64 start, u64 end) {
  return (u64)name_len + 3u + dec_digits(start) + dec_digits(end);
}
struct ScanFixRows {
  const K29Rec* recs;
  __device__ u64 operator()(u32 k) const { return paf_fix_row_len(recs[k]); }
};
template <bool TARGET>
struct ScanFixList {
  const K29Rec* recs;
  const wga_paf_line_dev* lines;
  __device__ u64 operator()(u32 k) const {
    const K29Rec& r = recs[k];
    if (!(r.flags & (TARGET ? WGA_PAF_FIX_TBAD : WGA_PAF_FIX_QBAD))) return 0u;
    const wga_paf_line_dev& L = lines[r.line];
    return TARGET ? paf_fix_item_len(L.tname_len, L.num[4], L.num[5]) : paf_fix_item_len(L.qname_len, L.num[1], L.num[2]);
  }
};
struct ScanFixBad { /* bad query ends | bad target ends << 32 */
  const K29Rec* recs;
  __device__ u64 operator()(u32 k) const {
    const u32 f = recs[k].flags;
    return (u64)(f & WGA_PAF_FIX_QBAD ? 1u : 0u) | ((u64)(f & WGA_PAF_FIX_TBAD ? 1u : 0u) << 32);
  }
};

/* ---- fix: fill --------------------------------------------------------------------------------------------------------------- */
/* one tile of the rows (blockIdx.x, 256 threads): records [0, nr), O their rows' places, `total` bytes in all */
__global__ __launch_bounds__(256) void k_paf_fix_fill(const u8* __restrict__ text, const K29Rec* __restrict__ recs,
                                                      const u64* __restrict__ O, u32 nr, u64 total, u8* __restrict__ out) {
  __shared__ u32x4_a16 s_tile[WGA_PAF_FIX_TILE / 16u];
  __shared__ u32 s_lo[3u * WGA_PAF_FIX_TILE_LINES], s_hi[3u * WGA_PAF_FIX_TILE_LINES];
  __shared__ u64 s_src[3u * WGA_PAF_FIX_TILE_LINES];
  __shared__ u32 s_first, s_count;
  u8* const tbuf = (u8*)s_tile;
  const u32 tid = threadIdx.x;
  const u64 T0 = (u64)blockIdx.x * WGA_PAF_FIX_TILE;
  const u32 tl = (u32)(total - T0 < WGA_PAF_FIX_TILE ? total - T0 : WGA_PAF_FIX_TILE);
  if (tid == 0u) {
    const u32 l0 = maf_find(O, nr, T0);
    const u32 lim = nr - l0 < WGA_PAF_FIX_TILE_LINES ? nr : l0 + WGA_PAF_FIX_TILE_LINES;
    s_first = l0;
    s_count = maf_find_in(O, l0, lim, T0 + tl - 1u) - l0 + 1u;
  }
  __syncthreads();
  const u32 l0 = s_first, nl = s_count; /* nl <= WGA_PAF_FIX_TILE_LINES */
  for (u32 j = tid; j < nl; j += 256u) {
    const K29Rec r = recs[l0 + j];
    MafClip c;
    c.buf = tbuf;
    c.tl = tl;
    /* the row's five parts: [0, f4b) of the line, eq, [f4e, f9b), et, [f9e, len); `at` = the part's place in the tile */
    long long at = (long long)(O[l0 + j] - T0);
    const u32 from[3] = {0u, r.f4e, r.f9e}, upto[3] = {r.f4b, r.f9b, r.len};
#pragma unroll
    for (u32 p = 0; p < 3u; p++) {
      const long long s0 = at, s1 = at + (long long)(upto[p] - from[p]);
      const long long lo = s0 < 0 ? 0 : s0 > (long long)tl ? (long long)tl : s0;
      const long long hi = s1 < 0 ? 0 : s1 > (long long)tl ? (long long)tl : s1;
      s_lo[3u * j + p] = (u32)lo;
      s_hi[3u * j + p] = (u32)hi;
      s_src[3u * j + p] = r.src + from[p] + (u64)(lo - s0);
      c.at = s1;
      if (p == 0u && (r.flags & WGA_PAF_FIX_QBAD)) c.num(r.eq);
      if (p == 1u && (r.flags & WGA_PAF_FIX_TBAD)) c.num(r.et);
      if (p == 2u) c.put((u8)0x0Au);
      at = c.at;
    }
  }
  __syncthreads();
  maf_tile_slices(tbuf, tl, 3u * nl, s_lo, s_hi, s_src, text, tid);
  __syncthreads();
  lds_text_flush(tbuf, 0u, tl, out + T0, tid, 256u);
}

/* ---- fix: lists -------------------------------------------------------------------------------------------------------------- */
__device__ __forceinline__ void paf_fix_item_put(u8* p, const u8* __restrict__ name, u32 name_len, u64 start, u64 end) {
  TextPut w = {p};
  w.str(name, name_len);
  w.c((u8)':');
  w.dec(start);
  w.c((u8)'-');
  w.dec(end);
  w.c((u8)0x0Au);
}

/* one thread per record; QB / TB = the scans of the two lists' item sizes; an item is written only into a span of its own size
 * inside its list (a scan that is not this call's writes nothing outside the lists); a null list is not written */
__global__ __launch_bounds__(256) void k_paf_fix_lists(const u8* __restrict__ text, const wga_paf_line_dev* __restrict__ lines,
                                                       const K29Rec* __restrict__ recs, u32 nr, const u64* __restrict__ QB,
                                                       const u64* __restrict__ TB, u64 q_total, u64 t_total,
                                                       u8* __restrict__ qlist, u8* __restrict__ tlist) {
  const u64 k = (u64)blockIdx.x * 256u + threadIdx.x;
  if (k >= nr) return;
  const K29Rec& r = recs[k];
  if (!r.flags) return;
  const wga_paf_line_dev& L = lines[r.line];
  if (qlist && (r.flags & WGA_PAF_FIX_QBAD)) {
    const u64 a = QB[k], b = QB[k + 1u];
    if (b <= q_total && b > a && b - a == paf_fix_item_len(L.qname_len, L.num[1], L.num[2]))
      paf_fix_item_put(qlist + a, text + L.qname_off, L.qname_len, L.num[1], L.num[2]);
  }
  if (tlist && (r.flags & WGA_PAF_FIX_TBAD)) {
    const u64 a = TB[k], b = TB[k + 1u];
    if (b <= t_total && b > a && b - a == paf_fix_item_len(L.tname_len, L.num[4], L.num[5]))
      paf_fix_item_put(tlist + a, text + L.tname_off, L.tname_len, L.num[4], L.num[5]);
  }
}

#endif /* WGA_K29_PAF_FIX_H */
