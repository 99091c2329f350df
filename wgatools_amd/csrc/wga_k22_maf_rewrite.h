/*
 * wga_k22_maf_rewrite.h — K22: `filter` and `rename` on MAF (tools/filter.rs:65-105, tools/rename.rs, MAFRecord::rename
 * parser/maf.rs:250-261, the writer maf.rs:566-581).  A call works on a WINDOW of consecutive blocks and writes every block
 * that survives as the reference's writer does: "a score=255\n", one line "s\t<prefix><name>\t<start>\t<size>\t<+|->\t<srcSize>
 * \t<text>\n" per row, an empty line.  start, size and srcSize are the input fields (size is NOT recounted: that is chunk's job).
 * Passes:
 *   select   one thread per block, from the row table alone: dropped under `filter` when the first row's size field is below
 *            min_block_size or the second row's srcSize field below min_query_size (filter.rs:96-101); BAD when `filter` is set
 *            and the block has fewer than two rows (the reference indexes slines[1] first: maf.rs:430) or when prefixes are
 *            given and the block's row count differs from theirs (maf.rs:252-254).  The smallest bad block is a global atomic
 *            min; the call's text is that of the blocks in front of it.
 *   compact  exclusive scan of the keep flags (blocks from the first bad one on count as dropped) = every kept block's place in
 *            the list of kept blocks; exclusive scan of that list's row counts = every kept block's first line.  The lines are
 *            numbered over kept blocks only: every numbered line holds 12 bytes or more, which K20's tile bookkeeping needs.
 *   lines    line lengths, their exclusive scan = every line's place in the text.
 *   fill     K20's tiles: 8 KiB of text per block in LDS, short fields through K20Clip (the name as prefix, then name: either
 *            may straddle a tile edge), the row texts in 16-byte groups (k20_tile_slices), lds_text_flush.  A row of 10^8
 *            columns is 12 000 tiles, spread over the grid like any other text.
 * No pass but the fill reads a row byte.  Traffic: the kept rows' bytes once in, the text once out, 12 bytes per block and 16
 * per line of tables.  The scans run over the window's blocks and lines, kept or not (the counts of kept ones stay on the
 * device until the count call's one read-back at its end).
 */
#ifndef WGA_K22_MAF_REWRITE_H
#define WGA_K22_MAF_REWRITE_H

#include "wga_k20_maf_chunk.h" /* k20_find, k20_find_in, K20Clip, k20_tile_slices, WGA_K20_TILE, WGA_K20_TILE_LINES */

struct K22Hdr {
  u32 first_bad; /* the first bad block, ~0u when there is none */
  u32 pad[3];
};

__global__ __launch_bounds__(256) void k_maf_rewrite_select(const wga_maf_slice_row* __restrict__ rows,
                                                            const wga_maf_rewrite_block* __restrict__ blocks, u32 nb,
                                                            wga_maf_rewrite_params P, u32* __restrict__ keep,
                                                            K22Hdr* __restrict__ hdr) {
  const u32 b = blockIdx.x * 256u + threadIdx.x;
  if (b >= nb) return;
  const wga_maf_rewrite_block B = blocks[b];
  const bool bad = (P.filter && B.n_rows < 2u) || (P.n_prefix && B.n_rows != P.n_prefix);
  bool k = !bad && B.n_rows != 0u;
  if (k && P.filter) /* filter.rs:100: both compare with `<` */
    k = !(rows[B.row0].size < P.min_block_size || rows[B.row0 + 1u].src_size < P.min_query_size);
  keep[b] = k ? 1u : 0u;
  if (bad) atomicMin(&hdr->first_bad, b);
}

/* scan functors: the blocks that are written; the rows of the j-th of them (0 behind the list's end, which kidx[nb] holds) */
struct ScanRewriteKept {
  const u32* keep;
  const K22Hdr* hdr;
  __device__ u64 operator()(u32 b) const { return keep[b] && b < hdr->first_bad ? 1u : 0u; }
};
struct ScanRewriteRows {
  const wga_maf_rewrite_block* blocks;
  const u32* klist;
  const u64* n_kept;
  __device__ u64 operator()(u32 j) const { return j < *n_kept ? blocks[klist[j]].n_rows : 0u; }
};

__global__ __launch_bounds__(256) void k_maf_rewrite_compact(const u64* __restrict__ kidx, u32 nb, u32* __restrict__ klist) {
  const u32 b = blockIdx.x * 256u + threadIdx.x;
  if (b >= nb) return;
  if (kidx[b + 1u] != kidx[b]) klist[kidx[b]] = b;
}

/* the line at index x of the kept lines: its row, its place in its block, the block's rows; x's block is kept block [jlo, jhi) */
struct K22Line {
  u32 r, n_rows, plen;
  u64 poff;
  wga_maf_slice_row row;
};
__device__ __forceinline__ K22Line k22_line(const wga_maf_slice_row* rows, const wga_maf_rewrite_block* blocks, const u32* klist,
                                            const u64* kline, u32 jlo, u32 jhi, const wga_maf_rewrite_params& P, u64 x) {
  K22Line l;
  const u32 j = k20_find_in(kline, jlo, jhi, x);
  const wga_maf_rewrite_block B = blocks[klist[j]];
  l.r = (u32)(x - kline[j]);
  l.n_rows = B.n_rows;
  l.row = rows[B.row0 + l.r];
  l.poff = 0u;
  l.plen = 0u;
  if (P.n_prefix) { /* a kept block has n_prefix rows */
    l.poff = P.d_prefix_off[l.r];
    l.plen = P.d_prefix_off[l.r + 1u] - P.d_prefix_off[l.r];
  }
  return l;
}
__device__ __forceinline__ u64 k22_line_len(const K22Line& l) {
  return (l.r == 0u ? 12u : 0u) + 2u + l.plen + l.row.name_len + 1u + dec_digits(l.row.start) + 1u + dec_digits(l.row.size) + 3u +
         dec_digits(l.row.src_size) + 1u + l.row.seq_len + (l.r + 1u == l.n_rows ? 2u : 1u);
}

/* lengths of the window's n line slots: the kept lines [0, kline[nb]) hold text, the slots behind them none */
__global__ __launch_bounds__(256) void k_maf_rewrite_lines(const wga_maf_slice_row* __restrict__ rows,
                                                           const wga_maf_rewrite_block* __restrict__ blocks, u32 nb,
                                                           const u32* __restrict__ klist, const u64* __restrict__ kidx,
                                                           const u64* __restrict__ kline, wga_maf_rewrite_params P, u32 n,
                                                           u64* __restrict__ len) {
  const u32 x = blockIdx.x * 256u + threadIdx.x;
  if (x >= n) return;
  if (x >= kline[nb]) {
    len[x] = 0u;
    return;
  }
  len[x] = k22_line_len(k22_line(rows, blocks, klist, kline, 0u, (u32)kidx[nb], P, x));
}

/* ---- fill: one 8 KiB tile of the text per block (k_maf_chunk_fill's scheme) ----------------------------------------------- */
__global__ __launch_bounds__(256) void k_maf_rewrite_fill(const u8* __restrict__ text, const wga_maf_slice_row* __restrict__ rows,
                                                          const wga_maf_rewrite_block* __restrict__ blocks, u32 nb,
                                                          const u32* __restrict__ klist, u32 nk, const u64* __restrict__ kline,
                                                          wga_maf_rewrite_params P, const u64* __restrict__ line_off, u64 total,
                                                          u8* __restrict__ out) {
  __shared__ u32x4_a16 s_tile[WGA_K20_TILE / 16u];
  __shared__ u32 s_lo[WGA_K20_TILE_LINES], s_hi[WGA_K20_TILE_LINES];
  __shared__ u64 s_src[WGA_K20_TILE_LINES];
  __shared__ u32 s_first, s_count, s_jlo, s_jhi;
  u8* const tbuf = (u8*)s_tile;
  const u32 tid = threadIdx.x;
  const u32 n = (u32)kline[nb]; /* the kept lines: the empty slots behind them start at `total` and are never among a tile's */
  const u64 T0 = (u64)blockIdx.x * WGA_K20_TILE;
  const u32 tl = (u32)(total - T0 < WGA_K20_TILE ? total - T0 : WGA_K20_TILE);
  if (tid == 0u) { /* the tile's lines [l0, l1] and their kept blocks [jlo, jhi): the lines' own block searches stay short */
    const u32 l0 = k20_find(line_off, n, T0);
    const u32 lim = n - l0 < WGA_K20_TILE_LINES ? n : l0 + WGA_K20_TILE_LINES;
    const u32 l1 = k20_find_in(line_off, l0, lim, T0 + tl - 1u);
    const u32 jlo = k20_find(kline, nk, l0);
    const u32 jlim = nk - jlo < l1 - l0 + 1u ? nk : jlo + (l1 - l0 + 1u); /* a kept block holds at least one line */
    s_first = l0;
    s_count = l1 - l0 + 1u;
    s_jlo = jlo;
    s_jhi = k20_find_in(kline, jlo, jlim, l1) + 1u;
  }
  __syncthreads();
  const u32 l0 = s_first, nl = s_count, jlo = s_jlo, jhi = s_jhi; /* nl <= WGA_K20_TILE_LINES: a line holds 12 bytes or more */
  for (u32 j = tid; j < nl; j += 256u) {
    const K22Line l = k22_line(rows, blocks, klist, kline, jlo, jhi, P, (u64)l0 + j);
    K20Clip c;
    c.buf = tbuf;
    c.at = (long long)(line_off[l0 + j] - T0);
    c.tl = tl;
    if (l.r == 0u) {
      const char* a = "a score=255\n";
      for (u32 e = 0; e < 12u; e++) c.put((u8)a[e]);
    }
    c.put((u8)'s');
    c.put((u8)'\t');
    /* prefix, then name: two spans of other memory behind each other; what lies in front of or behind the tile is skipped */
    const u8* part[2] = {P.d_prefix_text + l.poff, text + l.row.name_off};
    const u32 part_len[2] = {l.plen, l.row.name_len};
    for (u32 k = 0; k < 2u; k++) {
      const long long end = c.at + (long long)part_len[k];
      u32 e = c.at < 0 ? (u32)(-c.at < (long long)part_len[k] ? -c.at : (long long)part_len[k]) : 0u;
      c.at += (long long)e;
      for (; e < part_len[k] && c.at < (long long)tl; e++) c.put(part[k][e]);
      c.at = end;
    }
    c.put((u8)'\t');
    c.num(l.row.start);
    c.put((u8)'\t');
    c.num(l.row.size);
    c.put((u8)'\t');
    c.put(l.row.strand_neg ? (u8)'-' : (u8)'+');
    c.put((u8)'\t');
    c.num(l.row.src_size);
    c.put((u8)'\t');
    const long long s0 = c.at, s1 = c.at + (long long)l.row.seq_len;
    const long long lo = s0 < 0 ? 0 : s0 > (long long)tl ? (long long)tl : s0;
    const long long hi = s1 < 0 ? 0 : s1 > (long long)tl ? (long long)tl : s1;
    s_lo[j] = (u32)lo;
    s_hi[j] = (u32)hi;
    s_src[j] = l.row.seq_off + (u64)(lo - s0);
    c.at = s1;
    c.put((u8)'\n');
    if (l.r + 1u == l.n_rows) c.put((u8)'\n');
  }
  __syncthreads();
  k20_tile_slices(tbuf, tl, nl, s_lo, s_hi, s_src, text, tid);
  __syncthreads();
  lds_text_flush(tbuf, 0u, tl, out + T0, tid, 256u);
}

#endif /* WGA_K22_MAF_REWRITE_H */
