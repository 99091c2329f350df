/*
 * wga_maf_write.h — the MAF record writer of K20 (chunk), K21 (maf-ext) and K22 (filter, rename): the reference's writer
 * (maf.rs:566-581) on the device.  A record is "a score=255\n", one line "s\t<prefix><name>\t<start>\t<size>\t<+|->\t<srcSize>\t
 * <slice>\n" per row and an empty line.  A command numbers its window's lines in output order, describes line x as a MafLine
 * and needs two passes of its own around this header:
 *   lines   maf_line_len of every line; the exclusive scan of the lengths (line_off) = every line's place in the text.
 *   fill    maf_fill_tile: the text in 8 KiB TILES, one per block.  Thread 0 finds the tile's lines [l0, l1] in line_off and
 *           has the command narrow the range of their OWNERS (blocks, hits: what a line is looked up in), so that the lines'
 *           own searches stay short.  The block's threads write the short fields of the tile's lines into an LDS image of the
 *           tile (MafClip drops what falls outside it; decimal fields by dec_digits / dec_write; prefix and name are
 *           spans of other memory, either may straddle a tile edge), the slices are copied into the image in 16-byte groups
 *           (one unaligned 16-byte load + one aligned LDS store when a group lies inside one slice, bytes at slice ends), and
 *           the tile leaves in 16-byte stores (lds_text_flush).  A row of 10^8 columns is 12 000 tiles, spread over the grid
 *           like any other text.
 * A command supplies the fill with a line SOURCE: a trivially copyable struct of pointers and scalars with
 *   MafOwners owners(u32 l0, u32 l1) const       the owners of lines [l0, l1] (thread 0 only)
 *   MafLine line(MafOwners o, u64 x) const       line x, whose owner lies in o
 */
#ifndef WGA_MAF_WRITE_H
#define WGA_MAF_WRITE_H

#include "wga_text_out.h" /* dec_digits, dec_write, lds_text_flush */

#define WGA_MAF_TILE 8192u /* bytes of text per fill block */
/* lines one tile can meet: a line holds at least 11 bytes (the shortest, an empty name and slice and three one-digit numbers,
 * holds 12), so ceil(8192 / 11) + 1 = 746.  Lines without text (behind a panic, or of dropped blocks) start at the text's end
 * and are never among a tile's. */
#define WGA_MAF_TILE_LINES 768u

/* the last index i in [lo, hi) with base[i] <= x (base[lo] <= x) */
__device__ __forceinline__ u32 maf_find_in(const u64* base, u32 lo, u32 hi, u64 x) {
  while (hi - lo > 1u) {
    const u32 mid = (lo + hi) >> 1;
    if (base[mid] <= x)
      lo = mid;
    else
      hi = mid;
  }
  return lo;
}
__device__ __forceinline__ u32 maf_find(const u64* base, u32 n, u64 x) { return maf_find_in(base, 0u, n, x); }

struct MafOwners {
  u32 lo, hi;
};
/* the owners [lo, hi) of lines [l0, l1], first[i] being owner i's first line (n owners).  dense: every owner holds a line, so
 * the last one lies within l1 - l0 + 1 owners of the first; otherwise owners without lines share their successor's first line
 * and the last of them owns it */
__device__ __forceinline__ MafOwners maf_owners(const u64* first, u32 n, u32 l0, u32 l1, bool dense) {
  MafOwners o;
  o.lo = maf_find(first, n, l0);
  const u32 lim = dense && n - o.lo >= l1 - l0 + 1u ? o.lo + (l1 - l0 + 1u) : n;
  o.hi = maf_find_in(first, o.lo, lim, l1) + 1u;
  return o;
}

struct MafLine {
  u32 r, n_rows;    /* the row's index within its record, the record's rows */
  const u8* prefix; /* written in front of the name (prefix_len = 0: none) */
  u32 prefix_len, name_len;
  u64 name_off; /* the name: text[name_off .. name_off + name_len) */
  u64 start, size, src_size;
  u32 strand_neg;
  u64 src, width; /* the slice: text[src .. src + width) */
};
/* "a score=255\n" in front of a record's first row, the fields and their tabs, the slice, "\n", and the record's empty line
 * behind its last row: byte for byte what maf_fill_tile writes */
__device__ __forceinline__ u64 maf_line_len(const MafLine& l) {
  return (l.r == 0u ? 12u : 0u) + 2u + l.prefix_len + l.name_len + 1u + dec_digits(l.start) + 1u + dec_digits(l.size) + 3u +
         dec_digits(l.src_size) + 1u + l.width + (l.r + 1u == l.n_rows ? 2u : 1u);
}

struct MafClip { /* writes into the tile image, dropping what falls outside it */
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
  /* a span of other memory: what lies in front of or behind the tile is skipped, not walked */
  __device__ __forceinline__ void span(const u8* p, u32 len) {
    const long long end = at + (long long)len;
    u32 e = at < 0 ? (u32)(-at < (long long)len ? -at : (long long)len) : 0u;
    at += (long long)e;
    for (; e < len && at < (long long)tl; e++) put(p[e]);
    at = end;
  }
};
/* the slices of a tile's lines into its image, 16-byte group by group (line j's slice is [lo[j], hi[j]) of the tile, its bytes
 * start at text + src[j]): the first line whose slice ends behind the group's start, then the lines from there */
__device__ __forceinline__ void maf_tile_slices(u8* tbuf, u32 tl, u32 nl, const u32* s_lo, const u32* s_hi, const u64* s_src,
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

/* one tile of the text (blockIdx.x, 256 threads): lines [0, n) with text, line_off their places, `total` bytes in all */
template <typename Src>
__device__ __forceinline__ void maf_fill_tile(const Src& src, const u8* __restrict__ text, const u64* __restrict__ line_off,
                                              u32 n, u64 total, u8* __restrict__ out) {
  __shared__ u32x4_a16 s_tile[WGA_MAF_TILE / 16u];
  __shared__ u32 s_lo[WGA_MAF_TILE_LINES], s_hi[WGA_MAF_TILE_LINES];
  __shared__ u64 s_src[WGA_MAF_TILE_LINES];
  __shared__ u32 s_first, s_count, s_olo, s_ohi;
  u8* const tbuf = (u8*)s_tile;
  const u32 tid = threadIdx.x;
  const u64 T0 = (u64)blockIdx.x * WGA_MAF_TILE;
  const u32 tl = (u32)(total - T0 < WGA_MAF_TILE ? total - T0 : WGA_MAF_TILE);
  if (tid == 0u) {
    const u32 l0 = maf_find(line_off, n, T0);
    const u32 lim = n - l0 < WGA_MAF_TILE_LINES ? n : l0 + WGA_MAF_TILE_LINES;
    const u32 l1 = maf_find_in(line_off, l0, lim, T0 + tl - 1u);
    const MafOwners o = src.owners(l0, l1);
    s_first = l0;
    s_count = l1 - l0 + 1u;
    s_olo = o.lo;
    s_ohi = o.hi;
  }
  __syncthreads();
  const u32 l0 = s_first, nl = s_count; /* nl <= WGA_MAF_TILE_LINES */
  MafOwners own;
  own.lo = s_olo;
  own.hi = s_ohi;
  for (u32 j = tid; j < nl; j += 256u) {
    const MafLine l = src.line(own, (u64)l0 + j);
    MafClip c;
    c.buf = tbuf;
    c.at = (long long)(line_off[l0 + j] - T0);
    c.tl = tl;
    if (l.r == 0u) {
      const char* a = "a score=255\n";
      for (u32 e = 0; e < 12u; e++) c.put((u8)a[e]);
    }
    c.put((u8)'s');
    c.put((u8)'\t');
    c.span(l.prefix, l.prefix_len);
    c.span(text + l.name_off, l.name_len);
    c.put((u8)'\t');
    c.num(l.start);
    c.put((u8)'\t');
    c.num(l.size);
    c.put((u8)'\t');
    c.put(l.strand_neg ? (u8)'-' : (u8)'+');
    c.put((u8)'\t');
    c.num(l.src_size);
    c.put((u8)'\t');
    /* the slice: [at, at + width) of the tile, clipped, with its source */
    const long long s0 = c.at, s1 = c.at + (long long)l.width;
    const long long lo = s0 < 0 ? 0 : s0 > (long long)tl ? (long long)tl : s0;
    const long long hi = s1 < 0 ? 0 : s1 > (long long)tl ? (long long)tl : s1;
    s_lo[j] = (u32)lo;
    s_hi[j] = (u32)hi;
    s_src[j] = l.src + (u64)(lo - s0);
    c.at = s1;
    c.put((u8)'\n');
    if (l.r + 1u == l.n_rows) c.put((u8)'\n');
  }
  __syncthreads();
  maf_tile_slices(tbuf, tl, nl, s_lo, s_hi, s_src, text, tid);
  __syncthreads();
  lds_text_flush(tbuf, 0u, tl, out + T0, tid, 256u);
}

#endif /* WGA_MAF_WRITE_H */
