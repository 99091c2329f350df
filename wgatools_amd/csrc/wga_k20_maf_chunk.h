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
 *   size    line lengths in record order, their exclusive scan = every line's place in the text.
 *   fill    the text in 8 KiB tiles: a block's threads write the short fields of the tile's lines into an LDS image of the
 *           tile (decimal fields by dec_digits / dec_write of K9), the row slices are copied into it in 16-byte groups (one
 *           unaligned 16-byte load + one aligned LDS store when a group lies inside one slice, bytes at slice ends), and the
 *           tile leaves in 16-byte stores (lds_text_flush).
 * Traffic: the row bytes of the window twice (count, fill), the text once, 8-32 bytes per line of tables.
 */
#ifndef WGA_K20_MAF_CHUNK_H
#define WGA_K20_MAF_CHUNK_H

#include "wga_kernels.h"
#include "wga_k3_maf.h" /* maf_nonzero7, maf_gather8, maf_cols_from, popc32 */
#include "wga_k9_bed.h" /* dec_digits, dec_write, lds_text_flush */

#define WGA_K20_SLOTS 2048u   /* items one wave step can touch: 64 granules x 32 columns, one column per item at L = 1 */
#define WGA_K20_TILE 8192u    /* bytes of text per fill block */
#define WGA_K20_TILE_LINES 768u /* lines one tile can meet: a line is at least 11 bytes, ceil(8192 / 11) + 1 = 746 */
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
/* the last index i in [lo, hi) with base[i] <= x (base[lo] <= x) */
__device__ __forceinline__ u32 k20_find_in(const u64* base, u32 lo, u32 hi, u64 x) {
  while (hi - lo > 1u) {
    const u32 mid = (lo + hi) >> 1;
    if (base[mid] <= x)
      lo = mid;
    else
      hi = mid;
  }
  return lo;
}
__device__ __forceinline__ u32 k20_find(const u64* base, u32 n, u64 x) { return k20_find_in(base, 0u, n, x); }

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
        b = k20_find(bgran, nb, g);
        found = true;
      }
      { /* forward to the lane's block: a short binary search over the next 64 blocks (a step moves a lane 64 granules: it
         * passes 64 blocks at most, unless blocks of no granule lie between — then a search over the rest) */
        const u32 lim = nb - b > 64u ? b + 64u : nb;
        b = bgran[lim] <= g ? k20_find_in(bgran, lim, nb, g) : k20_find_in(bgran, b, lim, g);
      }
      const K20Blk k = k20_blk(blocks, rows, b, L);
      const u64 gpr = (k.c_end - k.c_beg + 31u) >> 5, q = g - bgran[b], r = q / gpr, j = q - r * gpr;
      col0 = k.c_beg + 32u * j;
      ncols = (u32)(k.c_end - col0 < 32u ? k.c_end - col0 : 32u);
      const u8* p = text + rows[k.row0 + r].seq_off + col0;
      u32 y[8];
      if (ncols == 32u) {
        const u32x4_a1 a0 = *(const u32x4_a1*)p, a1 = *(const u32x4_a1*)(p + 16);
#pragma unroll
        for (int d = 0; d < 4; d++) y[d] = a0[d], y[4 + d] = a1[d];
      } else { /* the row's window ends inside these 32 columns: no byte behind it is read, the rest counts as gaps */
        u8 t[32];
        for (u32 e = 0; e < 32u; e++) t[e] = e < ncols ? p[e] : (u8)'-';
        for (int d = 0; d < 8; d++) y[d] = (u32)t[4 * d] | ((u32)t[4 * d + 1] << 8) | ((u32)t[4 * d + 2] << 16) | ((u32)t[4 * d + 3] << 24);
      }
#pragma unroll
      for (int d = 0; d < 8; d++) y[d] = maf_nonzero7(y[d] ^ 0x2D2D2D2Du);
      mask = maf_gather8(y);
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

/* the line at record-order index x: its block, row and chunk, row-major item, start and size */
struct K20Line {
  u32 b, r;
  u64 kk, item, start, size, c0, width;
  K20Blk k;
};
__device__ __forceinline__ K20Line k20_line(const wga_maf_chunk_row* rows, const wga_maf_chunk_block* blocks, u32 blo,
                                            u32 bhi, const u64* bitem, const u64* pre, const u64* carry, u64 L, u64 x) {
  K20Line l; /* x's block lies in [blo, bhi) */
  l.b = k20_find_in(bitem, blo, bhi, x);
  l.k = k20_blk(blocks, rows, l.b, L);
  const u64 q = x - bitem[l.b];
  l.kk = q / l.k.n_rows;
  l.r = (u32)(q - l.kk * l.k.n_rows);
  const u64 row_item0 = bitem[l.b] + (u64)l.r * l.k.nkw;
  l.item = row_item0 + l.kk;
  l.start = rows[l.k.row0 + l.r].start + carry[l.k.row0 + l.r] + (pre[l.item] - pre[row_item0]); /* sline_end_vec */
  l.size = pre[l.item + 1u] - pre[l.item];
  const u64 kabs = l.k.k_lo + l.kk;
  l.c0 = kabs * L;
  l.width = k20_chunk_end(kabs, L, l.k.bl) - l.c0;
  return l;
}
/* bytes in front of the slice ("a score=255\n" for a record's first row, "s\t<name>\t<start>\t<size>\t<strand>\t<srcSize>\t")
 * and behind it ("\n", and the record's empty line after its last row) */
__device__ __forceinline__ u64 k20_head_len(const K20Line& l, const wga_maf_chunk_row& row) {
  return (l.r == 0u ? 12u : 0u) + 2u + row.name_len + 1u + dec_digits(l.start) + 1u + dec_digits(l.size) + 3u +
         dec_digits(row.src_size) + 1u;
}
__device__ __forceinline__ u64 k20_tail_len(const K20Line& l) { return l.r + 1u == l.k.n_rows ? 2u : 1u; }

__global__ __launch_bounds__(256) void k_maf_chunk_lines(const wga_maf_chunk_row* __restrict__ rows,
                                                         const wga_maf_chunk_block* __restrict__ blocks, u32 nb,
                                                         const u64* __restrict__ bitem, const u64* __restrict__ pre,
                                                         const u64* __restrict__ carry, u64 L, u32 n, u64* __restrict__ len) {
  const u32 x = blockIdx.x * 256u + threadIdx.x;
  if (x >= n) return;
  const K20Line l = k20_line(rows, blocks, 0u, nb, bitem, pre, carry, L, x);
  const wga_maf_chunk_row row = rows[l.k.row0 + l.r];
  len[x] = k20_head_len(l, row) + l.width + k20_tail_len(l);
}

/* ---- fill: one 8 KiB tile of the text per block -------------------------------------------------------------------------- */
struct K20Clip { /* writes into the tile image, dropping what falls outside it */
  u8* buf;
  long long at;
  u32 tl;
  __device__ __forceinline__ void put(u8 ch) {
    if (at >= 0 && at < (long long)tl) buf[at] = ch;
    at++;
  }
  __device__ __forceinline__ void num(u64 v) {
    u8 d[20];
    const u32 nd = dec_digits(v);
    dec_write(d, v, nd);
    for (u32 e = 0; e < nd; e++) put(d[e]);
  }
};
/* the slices of a tile's lines into its image, 16-byte group by group (line j's slice is [lo[j], hi[j]) of the tile, its bytes
 * start at text + src[j]): the first line whose slice ends behind the group's start, then the lines from there; one unaligned
 * 16-byte load + one aligned LDS store when a group lies inside one slice, bytes at slice ends */
__device__ __forceinline__ void k20_tile_slices(u8* tbuf, u32 tl, u32 nl, const u32* s_lo, const u32* s_hi, const u64* s_src,
                                                const u8* __restrict__ text, u32 tid) {
  const u32 ng = (tl + 15u) >> 4;
  for (u32 gi = tid; gi < ng; gi += 256u) {
    const u32 a = 16u * gi, e = a + 16u < tl ? a + 16u : tl;
    u32 lo = 0u, hi = nl; /* first j with s_hi[j] > a */
    while (lo < hi) {
      const u32 mid = (lo + hi) >> 1;
      if (s_hi[mid] > a)
        hi = mid;
      else
        lo = mid + 1u;
    }
    u32 j = lo;
    if (j < nl && s_lo[j] <= a && s_hi[j] >= a + 16u) {
      *(u32x4_a16*)(tbuf + a) = *(const u32x4_a1*)(text + s_src[j] + (a - s_lo[j]));
      continue;
    }
    for (; j < nl && s_lo[j] < e; j++) {
      const u32 x0 = s_lo[j] > a ? s_lo[j] : a, x1 = s_hi[j] < e ? s_hi[j] : e;
      const u8* src = text + s_src[j] - s_lo[j];
      for (u32 x = x0; x < x1; x++) tbuf[x] = src[x];
    }
  }
}
__global__ __launch_bounds__(256) void k_maf_chunk_fill(const u8* __restrict__ text, const wga_maf_chunk_row* __restrict__ rows,
                                                        const wga_maf_chunk_block* __restrict__ blocks, u32 nb,
                                                        const u64* __restrict__ bitem, const u64* __restrict__ pre,
                                                        const u64* __restrict__ carry, u64 L, u32 n,
                                                        const u64* __restrict__ line_off, u8* __restrict__ out) {
  __shared__ u32x4_a16 s_tile[WGA_K20_TILE / 16u];
  __shared__ u32 s_lo[WGA_K20_TILE_LINES], s_hi[WGA_K20_TILE_LINES];
  __shared__ u64 s_src[WGA_K20_TILE_LINES];
  __shared__ u32 s_first, s_count, s_blo, s_bhi;
  u8* const tbuf = (u8*)s_tile;
  const u32 tid = threadIdx.x;
  const u64 total = line_off[n];
  const u64 T0 = (u64)blockIdx.x * WGA_K20_TILE;
  const u32 tl = (u32)(total - T0 < WGA_K20_TILE ? total - T0 : WGA_K20_TILE);
  if (tid == 0u) { /* the tile's lines [l0, l1] and their blocks [blo, bhi): the lines' own block searches stay short */
    const u32 l0 = k20_find(line_off, n, T0);
    const u32 lim = n - l0 < WGA_K20_TILE_LINES ? n : l0 + WGA_K20_TILE_LINES;
    const u32 l1 = k20_find_in(line_off, l0, lim, T0 + tl - 1u);
    const u32 blo = k20_find(bitem, nb, l0);
    const u32 blim = nb - blo < l1 - l0 + 1u ? nb : blo + (l1 - l0 + 1u); /* a block holds at least one line */
    s_first = l0;
    s_count = l1 - l0 + 1u;
    s_blo = blo;
    s_bhi = k20_find_in(bitem, blo, blim, l1) + 1u;
  }
  __syncthreads();
  const u32 l0 = s_first, nl = s_count, blo = s_blo, bhi = s_bhi; /* nl <= WGA_K20_TILE_LINES: a line holds 11 bytes or more */
  for (u32 j = tid; j < nl; j += 256u) {
    const K20Line l = k20_line(rows, blocks, blo, bhi, bitem, pre, carry, L, (u64)l0 + j);
    const wga_maf_chunk_row row = rows[l.k.row0 + l.r];
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
    const u8* name = text + row.name_off;
    const long long name_end = c.at + (long long)row.name_len;
    for (u32 e = 0; e < row.name_len && c.at < (long long)tl; e++) c.put(name[e]);
    c.at = name_end;
    c.put((u8)'\t');
    c.num(l.start);
    c.put((u8)'\t');
    c.num(l.size);
    c.put((u8)'\t');
    c.put(row.strand_neg ? (u8)'-' : (u8)'+');
    c.put((u8)'\t');
    c.num(row.src_size);
    c.put((u8)'\t');
    /* the slice: [at, at + width) of the tile, clipped, with its source */
    const long long s0 = c.at, s1 = c.at + (long long)l.width;
    const long long lo = s0 < 0 ? 0 : s0 > (long long)tl ? (long long)tl : s0;
    const long long hi = s1 < 0 ? 0 : s1 > (long long)tl ? (long long)tl : s1;
    s_lo[j] = (u32)lo;
    s_hi[j] = (u32)hi;
    s_src[j] = row.seq_off + l.c0 + (u64)(lo - s0);
    c.at = s1;
    c.put((u8)'\n');
    if (l.r + 1u == l.k.n_rows) c.put((u8)'\n');
  }
  __syncthreads();
  k20_tile_slices(tbuf, tl, nl, s_lo, s_hi, s_src, text, tid);
  __syncthreads();
  lds_text_flush(tbuf, 0u, tl, out + T0, tid, 256u);
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
