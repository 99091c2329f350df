/*
 * wga_k21_maf_slice.h — K21: `maf-ext` (tools/mafextra.rs:167-232, MAFSLine::get_col_coord parser/maf.rs:81-95,
 * MAFRecord::slice_block parser/maf.rs:223-248, the writer maf.rs:566-581).  A HIT is one block cut by one region: the block's
 * rows [row0, row0 + n_rows) of the row table, the anchor row `ord` (the row of the region's name) and the anchor's bases
 * [cut_lo, cut_hi) counted from its start field; or the block as it is (`whole`).  col(p) = the column of the anchor's p-th
 * non-gap byte, the anchor's length when it has none; the hit's columns are [c0, c1) = [col(cut_lo), col(cut_hi)): every row is
 * written with that slice of its text, start = its start + cut_lo (plain addition for every row: for the anchor that is the
 * region's start, for the others the reference's quirk), size = cut_hi - cut_lo for the anchor and the slice's non-gap bytes
 * for the others.  A row shorter than c1 is the reference's slice panic: the call's text ends in front of the first such hit.
 * Many hits may name one block; nothing is kept between calls.  Passes:
 *   rank    the non-gap count of every 2048-column STRETCH of every table row (one wave step: 64 lanes x one 32-column mask in
 *           K3's bit order).  The stretches of all rows are one index space that the grid's waves share in contiguous runs, so a
 *           10^8-column row is spread over every wave.  Row r owns ceil(len / 2048) + 1 entries, the last one holds 0: the
 *           exclusive scan of all entries (wga's three-kernel scan) is then every row's rank directory, a row's rank at column
 *           2048 j being the difference of entry j and the row's entry 0.
 *   select  one wave per hit: col(p) = a binary search in the anchor's directory, then one wave step in the stretch found (lane
 *           popcounts, a wave prefix, a bit select inside the lane's mask); every other row's non-gap bytes over [c0, c1) = two
 *           ranks, each a directory difference plus one partial-stretch wave step.  The cost of a hit depends on its rows, not
 *           on the block's or the slice's length.  The short-row test is here (a global atomic min of the hit index).
 *   lines, fill   the record writer of wga_maf_write.h over the lines in hit order.
 * Traffic: the table rows once (rank), 2 x 2 KiB per row of a hit at most (select), the slices once and the text once (fill),
 * 8 bytes per stretch and 24 per line of tables.
 */
#ifndef WGA_K21_MAF_SLICE_H
#define WGA_K21_MAF_SLICE_H

#include "wga_k3_maf.h" /* maf_nongap_mask32, maf_cols_from, popc32 */
#include "wga_maf_write.h"

#define WGA_K21_STRETCH 2048u /* columns of one directory entry = one wave step */
#ifndef WGA_K21_GRID
#ifdef WGA_EMU
#define WGA_K21_GRID 3u
#else
#define WGA_K21_GRID 2048u /* rank blocks (4 waves each): eight per CU, every wave walks a contiguous run of stretches */
#endif
#endif

struct K21Hdr {
  u32 first_short; /* the first hit with a short row, ~0u when there is none */
  u32 pad[3];
};

/* scan functors: a row's directory entries, a hit's lines */
struct ScanSliceDir {
  const wga_maf_slice_row* rows;
  __device__ u64 operator()(u32 r) const { return ((rows[r].seq_len + (WGA_K21_STRETCH - 1u)) / WGA_K21_STRETCH) + 1u; }
};
struct ScanSliceLines {
  const wga_maf_slice_hit* hits;
  __device__ u64 operator()(u32 h) const { return hits[h].n_rows; }
};

/* ---- rank: the non-gap count of every stretch --------------------------------------------------------------------------- */
__global__ __launch_bounds__(256) void k_maf_slice_rank(const u8* __restrict__ text, const wga_maf_slice_row* __restrict__ rows,
                                                        u32 n_rows, const u64* __restrict__ dbase, u64* __restrict__ raw) {
  const u32 lane = threadIdx.x & 63u, w = WGA_WAVE_ID(threadIdx.x);
  const u64 E = dbase[n_rows], nwaves = (u64)gridDim.x * 4u, wid = (u64)blockIdx.x * 4u + w;
  const u64 x0 = E * wid / nwaves, x1 = E * (wid + 1u) / nwaves;
  if (x0 >= x1) return;
  u32 r = maf_find(dbase, n_rows, x0); /* the entry's row; later entries are reached by walking forward */
  for (u64 x = x0; x < x1; x++) {
    while (x >= dbase[r + 1u]) r++;
    const u64 j = x - dbase[r];
    const wga_maf_slice_row row = rows[r];
    const u32 c = popc32(maf_nongap_mask32(text + row.seq_off, row.seq_len, j * WGA_K21_STRETCH + 32u * lane)); /* 0 for the row's last entry */
    const u32 s = wave_sum_u32(c);
    if (lane == 0u) raw[x] = s;
  }
}

/* the non-gap bytes of the row's columns [0, c), c <= its length: directory entry c / 2048 plus the partial stretch (wave) */
__device__ __forceinline__ u64 k21_rank(const u8* __restrict__ text, const wga_maf_slice_row& row, const u64* __restrict__ dir,
                                        u64 c, u32 lane) {
  const u64 j = c / WGA_K21_STRETCH, s0 = j * WGA_K21_STRETCH, lc = s0 + 32u * lane;
  u32 m = 0u;
  if (lc < c) {
    m = maf_nongap_mask32(text + row.seq_off, row.seq_len, lc);
    if (c - lc < 32u) m &= ~maf_cols_from((u32)(c - lc));
  }
  return dir[j] - dir[0] + wave_sum_u32(popc32(m));
}
/* get_col_coord (maf.rs:81-95): the column of the row's p-th non-gap byte, its length when it has p or fewer (wave) */
__device__ __forceinline__ u64 k21_select(const u8* __restrict__ text, const wga_maf_slice_row& row, const u64* __restrict__ dir,
                                          u32 nent, u64 p, u32 lane) {
  if (p >= dir[nent - 1u] - dir[0]) return row.seq_len;
  const u64 target = p + dir[0];
  const u32 j = maf_find(dir, nent - 1u, target); /* the last stretch whose rank is <= p: it holds the byte */
  const u32 rem = (u32)(target - dir[j]);
  const u64 lc = (u64)j * WGA_K21_STRETCH + 32u * lane;
  const u32 m = maf_nongap_mask32(text + row.seq_off, row.seq_len, lc), cnt = popc32(m);
  const u32 incl = wave_incl_scan_u32(cnt);
  const u64 ball = __ballot(incl > rem);
  const u32 src = (u32)__builtin_ctzll(ball); /* the lane that holds it (the stretch holds more than rem non-gap bytes) */
  u32 k = 0u;
  if (lane == src) { /* the largest k with fewer than q + 1 ... exactly: #non-gap in columns [0, k) <= q */
    const u32 q = rem - (incl - cnt);
    u32 lo = 0u, hi = 32u;
    while (hi - lo > 1u) {
      const u32 mid = (lo + hi) >> 1;
      if (popc32(m & ~maf_cols_from(mid)) <= q)
        lo = mid;
      else
        hi = mid;
    }
    k = lo;
  }
  k = wave_get_u32_dyn(k, src);
  return (u64)j * WGA_K21_STRETCH + 32u * src + k;
}

/* ---- select + count: one wave per hit ------------------------------------------------------------------------------------ */
__global__ __launch_bounds__(256) void k_maf_slice_select(const u8* __restrict__ text, const wga_maf_slice_row* __restrict__ rows,
                                                          const wga_maf_slice_hit* __restrict__ hits, u32 n_hits,
                                                          const u64* __restrict__ dbase, const u64* __restrict__ G,
                                                          const u64* __restrict__ hline, u64* __restrict__ C0,
                                                          u64* __restrict__ C1, u64* __restrict__ sz, K21Hdr* __restrict__ hdr) {
  const u32 lane = threadIdx.x & 63u;
  const u64 hw = (u64)blockIdx.x * 4u + WGA_WAVE_ID(threadIdx.x);
  if (hw >= n_hits) return;
  const u32 h = (u32)hw;
  const wga_maf_slice_hit H = hits[h];
  if (H.whole || H.n_rows == 0u) {
    if (lane == 0u) C0[h] = 0u, C1[h] = 0u;
    return;
  }
  const u64 ar = H.row0 + H.ord;
  const wga_maf_slice_row A = rows[ar];
  const u64* const adir = G + dbase[ar];
  const u32 anent = (u32)(dbase[ar + 1u] - dbase[ar]);
  const u64 c0 = k21_select(text, A, adir, anent, H.cut_lo, lane);
  const u64 c1 = k21_select(text, A, adir, anent, H.cut_hi, lane);
  if (lane == 0u) C0[h] = c0, C1[h] = c1;
  const u64 l0 = hline[h];
  bool is_short = false;
  for (u32 r = 0; r < H.n_rows; r++) {
    if (r == H.ord) continue;
    const wga_maf_slice_row R = rows[H.row0 + r];
    if (R.seq_len < c1) { /* maf.rs:240: the slice panics */
      is_short = true;
      continue;
    }
    const u64* const dir = G + dbase[H.row0 + r];
    const u64 n = k21_rank(text, R, dir, c1, lane) - k21_rank(text, R, dir, c0, lane);
    if (lane == 0u) sz[l0 + r] = n;
  }
  if (is_short && lane == 0u) atomicMin(&hdr->first_short, h);
}

/* the window's lines in hit order: line x is row x - hline[h] of its hit h (the owner).  Hits without rows share their
 * successor's first line: the last one owns it */
struct K21Lines {
  const wga_maf_slice_row* rows;
  const wga_maf_slice_hit* hits;
  const u64 *hline, *C0, *C1, *sz;
  u32 n_hits;
  __device__ __forceinline__ MafOwners owners(u32 l0, u32 l1) const { return maf_owners(hline, n_hits, l0, l1, false); }
  __device__ __forceinline__ MafLine line(MafOwners o, u64 x) const {
    const u32 h = maf_find_in(hline, o.lo, o.hi, x);
    const wga_maf_slice_hit H = hits[h];
    MafLine l;
    l.r = (u32)(x - hline[h]);
    l.n_rows = H.n_rows;
    const wga_maf_slice_row row = rows[H.row0 + l.r];
    l.prefix = nullptr;
    l.prefix_len = 0u;
    l.name_off = row.name_off;
    l.name_len = row.name_len;
    l.src_size = row.src_size;
    l.strand_neg = row.strand_neg;
    if (H.whole) { /* mafextra.rs:205-208: the record as it was read */
      l.start = row.start;
      l.size = row.size;
      l.src = row.seq_off;
      l.width = row.seq_len;
    } else {
      l.start = row.start + H.cut_lo; /* maf.rs:229 for the anchor (= the region's start), maf.rs:239 for the others */
      l.size = l.r == H.ord ? H.cut_hi - H.cut_lo : sz[x];
      l.src = row.seq_off + C0[h];
      l.width = C1[h] - C0[h];
    }
    return l;
  }
};

/* lengths of the window's n lines: 0 from the first short hit on (the lines behind the panic hold no text, so they start at the
 * text's end) */
__global__ __launch_bounds__(256) void k_maf_slice_lines(const wga_maf_slice_row* __restrict__ rows,
                                                         const wga_maf_slice_hit* __restrict__ hits, u32 n_hits,
                                                         const u64* __restrict__ hline, const u64* __restrict__ C0,
                                                         const u64* __restrict__ C1, const u64* __restrict__ sz,
                                                         const K21Hdr* __restrict__ hdr, u32 n, u64* __restrict__ len) {
  const u32 x = blockIdx.x * 256u + threadIdx.x;
  if (x >= n) return;
  const u32 fs = hdr->first_short;
  if (fs != 0xFFFFFFFFu && x >= hline[fs]) {
    len[x] = 0u;
    return;
  }
  const K21Lines src = {rows, hits, hline, C0, C1, sz, n_hits};
  len[x] = maf_line_len(src.line(MafOwners{0u, n_hits}, x));
}

__global__ __launch_bounds__(256) void k_maf_slice_fill(const u8* __restrict__ text, const wga_maf_slice_row* __restrict__ rows,
                                                        const wga_maf_slice_hit* __restrict__ hits, u32 n_hits,
                                                        const u64* __restrict__ hline, const u64* __restrict__ C0,
                                                        const u64* __restrict__ C1, const u64* __restrict__ sz, u32 n,
                                                        const u64* __restrict__ line_off, u8* __restrict__ out) {
  const K21Lines src = {rows, hits, hline, C0, C1, sz, n_hits};
  maf_fill_tile(src, text, line_off, n, line_off[n], out);
}

#endif /* WGA_K21_MAF_SLICE_H */
