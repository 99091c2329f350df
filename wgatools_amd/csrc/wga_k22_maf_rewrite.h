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
 *            numbered over kept blocks only, so every numbered line holds text.
 *   lines, fill   the record writer of wga_maf_write.h over the kept lines; the name goes behind the row's prefix.
 * No pass but the fill reads a row byte.  Traffic: the kept rows' bytes once in, the text once out, 12 bytes per block and 16
 * per line of tables.  The scans run over the window's blocks and lines, kept or not (the counts of kept ones stay on the
 * device until the count call's one read-back at its end).
 */
#ifndef WGA_K22_MAF_REWRITE_H
#define WGA_K22_MAF_REWRITE_H

#include "wga_maf_write.h"

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

/* the kept lines in output order: line x is row x - kline[j] of the j-th kept block (the owner); every field is the row table's */
struct K22Lines {
  const wga_maf_slice_row* rows;
  const wga_maf_rewrite_block* blocks;
  const u32* klist;
  const u64* kline;
  wga_maf_rewrite_params P;
  u32 nk;
  __device__ __forceinline__ MafOwners owners(u32 l0, u32 l1) const { return maf_owners(kline, nk, l0, l1, true); }
  __device__ __forceinline__ MafLine line(MafOwners o, u64 x) const {
    const u32 j = maf_find_in(kline, o.lo, o.hi, x);
    const wga_maf_rewrite_block B = blocks[klist[j]];
    MafLine l;
    l.r = (u32)(x - kline[j]);
    l.n_rows = B.n_rows;
    const wga_maf_slice_row row = rows[B.row0 + l.r];
    l.prefix = nullptr;
    l.prefix_len = 0u;
    if (P.n_prefix) { /* a kept block has n_prefix rows */
      l.prefix = P.d_prefix_text + P.d_prefix_off[l.r];
      l.prefix_len = P.d_prefix_off[l.r + 1u] - P.d_prefix_off[l.r];
    }
    l.name_off = row.name_off;
    l.name_len = row.name_len;
    l.start = row.start;
    l.size = row.size;
    l.src_size = row.src_size;
    l.strand_neg = row.strand_neg;
    l.src = row.seq_off;
    l.width = row.seq_len;
    return l;
  }
};

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
  const K22Lines src = {rows, blocks, klist, kline, P, (u32)kidx[nb]};
  len[x] = maf_line_len(src.line(MafOwners{0u, src.nk}, x));
}

__global__ __launch_bounds__(256) void k_maf_rewrite_fill(const u8* __restrict__ text, const wga_maf_slice_row* __restrict__ rows,
                                                          const wga_maf_rewrite_block* __restrict__ blocks, u32 nb,
                                                          const u32* __restrict__ klist, u32 nk, const u64* __restrict__ kline,
                                                          wga_maf_rewrite_params P, const u64* __restrict__ line_off, u64 total,
                                                          u8* __restrict__ out) {
  const K22Lines src = {rows, blocks, klist, kline, P, nk};
  maf_fill_tile(src, text, line_off, (u32)kline[nb], total, out); /* the kept lines: the slots behind them hold no text */
}

#endif /* WGA_K22_MAF_REWRITE_H */
