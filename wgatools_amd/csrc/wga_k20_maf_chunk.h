/*
 * wga_k20_maf_chunk.h — K20: `chunk` on MAF (tools/chunk.rs:20-90, recount_align_size parser/common.rs:179-190, the writer
 * maf.rs:566-581).  Every block is cut into pieces of at most L columns of its FIRST row; every row of every piece is written
 * with its own start (the row's input start plus the non-gap bytes of its earlier pieces) and size (the non-gap bytes of the
 * piece).
 *
 * A call works on a WINDOW: consecutive chunk records of consecutive blocks (the host cuts a piece's records into windows of
 * bounded text).  A window's lines are numbered twice over the same range: row-major inside a block (item = row * nk + chunk,
 * what the counts and their scan use: a row's start is a difference of the scan) and record-major (line = chunk * n_rows + row,
 * the output order).  Passes:
 *   count   the window's row columns as 32-column GRANULES (a lane holds 32 consecutive columns of one row; a wave takes 64
 *           consecutive granules, so short rows share a wave and a 10^8-column row is spread over the whole grid); a lane's
 *           non-gap bytes are ONE 32-bit mask in K3's bit order (bit 8e + d = column 4d + e), a chunk's share of it one
 *           popcount under a range mask built in that order.  The shares go to per-wave LDS slots (one per item the wave
 *           touches), then leave once per item: a plain store for the items that lie wholly inside the wave's granules, a
 *           global atomic for the two at its ends (shared with the waves in front and behind).
 *   start   exclusive scan of the counts (wga's three-kernel scan); the row's carry from earlier windows (d_carry, the
 *           reference's sline_end_vec) is added where a line is formatted and advanced at the end of the fill call.
 *   lines, fill   the record writer of wga_maf_write.h over the lines in record order.
 * Traffic: the row bytes of the window twice (count, fill), the text once, 8-32 bytes per line of tables.
 */
#ifndef WGA_K20_MAF_CHUNK_H
#define WGA_K20_MAF_CHUNK_H

#include "wga_k3_maf.h" /* maf_nongap_mask32, maf_cols_from, popc32 */
#include "wga_maf_write.h"

#define WGA_K20_SLOTS 2048u   /* items one wave step can touch: 64 granules x 32 columns, one column per item at L = 1 */
#ifndef WGA_K20_GRID
#ifdef WGA_EMU
#define WGA_K20_GRID 3u
#else
#define WGA_K20_GRID 2048u /* count blocks (4 waves each): eight per CU, every wave walks a contiguous run of granule steps */
#endif
#endif

/* the block's window geometry */
struct K20Blk {
  u64 row0, k_lo, nkw, bl, c_beg, c_end;
  u32 n_rows;
};
/* end of chunk k (chunk.rs:43-56: [kL, kL + L) while that ends before the block's end, then the block's end) */
__device__ __forceinline__ u64 k20_chunk_end(u64 k, u64 L, u64 bl) {
  const u64 c0 = k * L;
  return bl - c0 > L ? c0 + L : bl;
}
__device__ __forceinline__ K20Blk k20_blk(const wga_maf_chunk_block* blocks, const wga_maf_chunk_row* rows, u32 b, u64 L) {
  const wga_maf_chunk_block B = blocks[b];
  K20Blk g;
  g.row0 = B.row0;
  g.k_lo = B.k_lo;
  g.nkw = B.k_hi - B.k_lo;
  g.n_rows = B.n_rows;
  g.bl = rows[B.row0].seq_len; /* chunk.rs:35: the first row sets the columns */
  g.c_beg = B.k_lo * L;
  g.c_end = k20_chunk_end(B.k_hi - 1u, L, g.bl);
  return g;
}
/* scan functors over the window's blocks: lines (n_rows * chunks) and 32-column granules (n_rows * ceil(columns / 32)) */
struct ScanChunkItems {
  const wga_maf_chunk_block* blocks;
  __device__ u64 operator()(u32 b) const { return (u64)blocks[b].n_rows * (blocks[b].k_hi - blocks[b].k_lo); }
};
struct ScanChunkGran {
  const wga_maf_chunk_block* blocks;
  const wga_maf_chunk_row* rows;
  u64 L;
  __device__ u64 operator()(u32 b) const {
    const K20Blk g = k20_blk(blocks, rows, b, L);
    return (u64)g.n_rows * ((g.c_end - g.c_beg + 31u) >> 5);
  }
};

/* ---- count: non-gap bytes of every (row, chunk) of the window ---------------------------------------------------------- */
__global__ __launch_bounds__(256) void k_maf_chunk_count(const u8* __restrict__ text, const wga_maf_chunk_row* __restrict__ rows,
                                                         const wga_maf_chunk_block* __restrict__ blocks, u32 nb,
                                                         const u64* __restrict__ bitem, const u64* __restrict__ bgran, u64 L,
                                                         u64* __restrict__ cnt) {
  __shared__ u32 s_slot[4u * WGA_K20_SLOTS];
  const u32 lane = threadIdx.x & 63u, w = WGA_WAVE_ID(threadIdx.x);
  u32* const slot = s_slot + w * WGA_K20_SLOTS;
  for (u32 s = lane; s < WGA_K20_SLOTS; s += 64u) slot[s] = 0u;
  WGA_WAVE_SYNC();
  /* every wave walks a contiguous run of 64-granule steps: a lane finds its block once and then moves forward (a search per
   * step was a chain of ~20 dependent loads in front of every step) */
  const u64 G = bgran[nb], nsteps = (G + 63u) >> 6, nwaves = (u64)gridDim.x * 4u, wid = (u64)blockIdx.x * 4u + w;
  const u64 st0 = nsteps * wid / nwaves, st1 = nsteps * (wid + 1u) / nwaves;
  u32 b = 0u;
  bool found = false;
  for (u64 st = st0; st < st1; st++) {
    const u64 g = 64u * st + lane;
    const bool valid = g < G;
    u64 item_a = 0u, item_z = 0u, col0 = 0u, kA = 0u, kZ = 0u, ibase = 0u;
    u32 mask = 0u, ncols = 0u;
    if (valid) {
      if (!found) {
        b = maf_find(bgran, nb, g);
        found = true;
      }
      { /* forward to the lane's block: a short binary search over the next 64 blocks (a step moves a lane 64 granules: it
         * passes 64 blocks at most, unless blocks of no granule lie between — then a search over the rest) */
        const u32 lim = nb - b > 64u ? b + 64u : nb;
        b = bgran[lim] <= g ? maf_find_in(bgran, lim, nb, g) : maf_find_in(bgran, b, lim, g);
      }
      const K20Blk k = k20_blk(blocks, rows, b, L);
      const u64 gpr = (k.c_end - k.c_beg + 31u) >> 5, q = g - bgran[b], r = q / gpr, j = q - r * gpr;
      col0 = k.c_beg + 32u * j;
      ncols = (u32)(k.c_end - col0 < 32u ? k.c_end - col0 : 32u);
      mask = maf_nongap_mask32(text + rows[k.row0 + r].seq_off, k.c_end, col0); /* columns behind the window's chunks are not read */
      kA = col0 / L;
      kZ = (col0 + ncols - 1u) / L;
      ibase = bitem[b] + r * k.nkw - k.k_lo;
      item_a = ibase + kA;
      item_z = ibase + kZ;
    }
    /* the wave's items: [first lane's first, last valid lane's last] (valid lanes are a prefix) */
    const u32 last = (u32)__popcll(__ballot(valid)) - 1u;
    const u64 wa = ((u64)wave_get_u32((u32)(item_a >> 32), 0) << 32) | (u64)wave_get_u32((u32)item_a, 0);
    const u64 wz = ((u64)wave_get_u32_dyn((u32)(item_z >> 32), last) << 32) | (u64)wave_get_u32_dyn((u32)item_z, last);
    const u64 span = wz - wa + 1u;
    const bool direct = span > WGA_K20_SLOTS; /* wave-uniform: empty blocks between (their items hold no granule) */
    if (valid) {
      for (u64 k = kA; k <= kZ; k++) {
        const u64 cb = k * L, ce = cb + L; /* the chunk's columns (its true end is past the lane's when it is the block's last) */
        const u32 lo = cb > col0 ? (u32)(cb - col0) : 0u;
        const u32 hi = ce - col0 < (u64)ncols && ce > col0 ? (u32)(ce - col0) : ncols;
        const u32 c = popc32(mask & maf_cols_from(lo) & ~maf_cols_from(hi));
        if (c) {
          if (direct)
            atomicAdd(&cnt[ibase + k], (u64)c);
          else
            atomicAdd(&slot[ibase + k - wa], c);
        }
      }
    }
    WGA_WAVE_SYNC();
    if (!direct) {
      for (u32 s = lane; s < (u32)span; s += 64u) {
        const u32 v = slot[s];
        if (v) {
          if (s == 0u || s + 1u == (u32)span)
            atomicAdd(&cnt[wa + s], (u64)v);
          else
            cnt[wa + s] = v; /* an item wholly inside this wave's granules */
          slot[s] = 0u;
        }
      }
    }
    WGA_WAVE_SYNC();
  }
}

/* the window's lines in record order: line x is row x % n_rows of record x / n_rows of its block (the owner); its start is the
 * row's input start, its carry from earlier windows and the counts of its chunks in front in this one (sline_end_vec) */
struct K20Lines {
  const wga_maf_chunk_row* rows;
  const wga_maf_chunk_block* blocks;
  const u64 *bitem, *pre, *carry;
  u64 L;
  u32 nb;
  __device__ __forceinline__ MafOwners owners(u32 l0, u32 l1) const { return maf_owners(bitem, nb, l0, l1, true); }
  __device__ __forceinline__ MafLine line(MafOwners o, u64 x) const {
    const u32 b = maf_find_in(bitem, o.lo, o.hi, x);
    const K20Blk k = k20_blk(blocks, rows, b, L);
    const u64 q = x - bitem[b], kk = q / k.n_rows, kabs = k.k_lo + kk, c0 = kabs * L;
    MafLine l;
    l.r = (u32)(q - kk * k.n_rows);
    l.n_rows = k.n_rows;
    const wga_maf_chunk_row row = rows[k.row0 + l.r];
    const u64 row_item0 = bitem[b] + (u64)l.r * k.nkw, item = row_item0 + kk; /* row-major */
    l.prefix = nullptr;
    l.prefix_len = 0u;
    l.name_off = row.name_off;
    l.name_len = row.name_len;
    l.start = row.start + carry[k.row0 + l.r] + (pre[item] - pre[row_item0]);
    l.size = pre[item + 1u] - pre[item];
    l.src_size = row.src_size;
    l.strand_neg = row.strand_neg;
    l.src = row.seq_off + c0;
    l.width = k20_chunk_end(kabs, L, k.bl) - c0;
    return l;
  }
};

__global__ __launch_bounds__(256) void k_maf_chunk_lines(const wga_maf_chunk_row* __restrict__ rows,
                                                         const wga_maf_chunk_block* __restrict__ blocks, u32 nb,
                                                         const u64* __restrict__ bitem, const u64* __restrict__ pre,
                                                         const u64* __restrict__ carry, u64 L, u32 n, u64* __restrict__ len) {
  const u32 x = blockIdx.x * 256u + threadIdx.x;
  if (x >= n) return;
  const K20Lines src = {rows, blocks, bitem, pre, carry, L, nb};
  len[x] = maf_line_len(src.line(MafOwners{0u, nb}, x));
}

__global__ __launch_bounds__(256) void k_maf_chunk_fill(const u8* __restrict__ text, const wga_maf_chunk_row* __restrict__ rows,
                                                        const wga_maf_chunk_block* __restrict__ blocks, u32 nb,
                                                        const u64* __restrict__ bitem, const u64* __restrict__ pre,
                                                        const u64* __restrict__ carry, u64 L, u32 n,
                                                        const u64* __restrict__ line_off, u8* __restrict__ out) {
  const K20Lines src = {rows, blocks, bitem, pre, carry, L, nb};
  maf_fill_tile(src, text, line_off, n, line_off[n], out);
}

/* the rows' carries advance by their chunks' sizes in this window (behind the fill, which read them) */
__global__ __launch_bounds__(256) void k_maf_chunk_carry(const wga_maf_chunk_block* __restrict__ blocks, u32 nb,
                                                         const u64* __restrict__ bitem, const u64* __restrict__ pre,
                                                         u64* __restrict__ carry) {
  const u32 b = blockIdx.x * 256u + threadIdx.x;
  if (b >= nb) return;
  const wga_maf_chunk_block B = blocks[b];
  const u64 nkw = B.k_hi - B.k_lo;
  for (u32 r = 0; r < B.n_rows; r++) {
    const u64 i0 = bitem[b] + (u64)r * nkw;
    carry[B.row0 + r] += pre[i0 + nkw] - pre[i0];
  }
}

#endif /* WGA_K20_MAF_CHUNK_H */
