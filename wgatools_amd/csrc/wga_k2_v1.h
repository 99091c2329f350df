/*
 * wga_k2_v1.h — v1 of the paf2maf row kernel (gap insertion, parse_cigar_to_insert), and the window, merge and granule-table
 * machinery that only it and K6's block kernel (wga_k6_pafpseudo.h) use.  The streaming kernel (wga_kernels_k2s.h) is the
 * default; v1 is `expand_variant` 0 and, as k_paf2maf_expand_list, the fallback for the tiles K2s leaves.
 *
 *   k_paf2maf_expand  one 256-thread block per tile; block scan of the tile's ops into LDS
 *                     (compacted per-row gap lists + a per-16-column granule table); every
 *                     lane then owns 16-column output granules: a table lookup says "plain
 *                     copy" (one byte-unaligned 16 B window load, reverse-complement fused for
 *                     '-' strand), "all dashes", or "touches a gap" (queued and assembled from
 *                     two windows under byte masks).  Raw buffer loads / stores with
 *                     out-of-range offsets as the lane predicate; no read-modify-write.
 *
 * The pre-pass it starts from (k_rec_desc, k_tile_base, wga_tile_desc), ExpandArgs and the byte helpers it shares with K2s are
 * in wga_kernels.h.
 */
#ifndef WGA_K2_V1_H
#define WGA_K2_V1_H

#include "wga_kernels.h"

#ifndef WGA_DRAIN_MIN
#define WGA_DRAIN_MIN 32u /* queued complex chunks that trigger a drain before the row ends: the rows of K2 take the value from
                             the host (ExpandArgs::drain_min), everything else this one.  64 fills the drain's lanes (fewest
                             instructions) but lets the lines its chunks belong to wait half written in the L2; 16 completes them
                             at once.  Same buffers, one process (scripts/gpu_k2_same_buffers.py): with 2 x 50 MB pools 64 / 32 /
                             16 = 6.19 / 6.44 / 6.66 ms, with 2 x 1 GB pools (the L2 churns with source lines) 8.65 / 8.07 / 7.85 */
#endif
#ifndef WGA_DRAIN_POOL_BYTES
#define WGA_DRAIN_POOL_BYTES (192ull << 20) /* sequence pools beyond this (together) do not stay in the 256 MB Infinity Cache */
#endif
struct RowSrc {
  const u8* fa;  /* sequence pool */
  u64 fa_bytes;  /* pool size (window loads are bounds-checked against it) */
  u64 src_off;   /* start of this record's slice in the pool */
  u64 src_len;   /* slice length as fetched */
  bool rc;       /* read reversed + complemented (utils.rs:83-101) */
  bool safe;     /* every 20-byte window of this row lies inside the pool (rowsrc_prepare) */
  u32 drain_min = WGA_DRAIN_MIN; /* queued complex chunks that trigger a drain before the row ends (see WGA_DRAIN_MIN) */
  const u8* win_base; /* address of slice index sbase (rc: of the mirrored window start) */
};

/* A 16-byte source window: output byte j of a chunk <-> slice index S + j (S may be negative /
 * beyond the slice for bytes outside the piece — those are masked by the caller).  Split in two
 * so that several windows can be in flight: win_issue only issues the load (ONE byte-aligned
 * global_load_dwordx4), win_finish — for rc — reverses + complements and flags invalid bases
 * (non-zero byte).  `off` = S - sbase is a small i32; the 64-bit part of the address is
 * wave-uniform (RowSrc::win_base).  Rows whose slice sits >= 32 bytes inside the pool (`safe`,
 * uniform) load unchecked; rows at a pool edge take guarded byte loads. */
struct WinRaw {
  u32 v[4];
};

__device__ __forceinline__ void win_issue(const RowSrc& src, u64 sbase, int off, int pa, int pb,
                                          WinRaw& r) {
  if (src.safe) {
    /* pointer arithmetic only (no integer round trip): keeps this a global_load, not flat */
    const int sgn = src.rc ? -1 : 0; /* uniform */
    const u8* p = src.win_base + (i64)((off ^ sgn) - sgn);
    u32x4_a1 v = *(const u32x4_a1*)p;
    r.v[0] = v[0];
    r.v[1] = v[1];
    r.v[2] = v[2];
    r.v[3] = v[3];
  } else { /* pool edge: guarded byte loads, only for the bytes of the piece */
    const i64 S = (i64)sbase + off;
    const i64 P = src.rc ? (i64)src.src_off + (i64)src.src_len - 16 - S : (i64)src.src_off + S;
    u64 lo = 0, hi = 0; /* no dynamically indexed array: that would force WinRaw into scratch */
    for (int j = pa; j < pb; j++) {
      int vj = src.rc ? 15 - j : j; /* position inside the address-ordered window */
      i64 idx = P + vj;
      u64 byte = (idx >= 0 && (u64)idx < src.fa_bytes) ? (u64)src.fa[idx] : 0ull;
      if (vj < 8)
        lo |= byte << (8 * vj);
      else
        hi |= byte << (8 * (vj - 8));
    }
    r.v[0] = (u32)lo;
    r.v[1] = (u32)(lo >> 32);
    r.v[2] = (u32)hi;
    r.v[3] = (u32)(hi >> 32);
  }
}

__device__ __forceinline__ void win_finish(const RowSrc& src, const WinRaw& r, u32 W[4],
                                           u32 inv[4]) {
  if (src.rc) {
    W[0] = comp4(bswap32(r.v[3]), &inv[0]);
    W[1] = comp4(bswap32(r.v[2]), &inv[1]);
    W[2] = comp4(bswap32(r.v[1]), &inv[2]);
    W[3] = comp4(bswap32(r.v[0]), &inv[3]);
  } else {
    W[0] = r.v[0];
    W[1] = r.v[1];
    W[2] = r.v[2];
    W[3] = r.v[3];
    inv[0] = inv[1] = inv[2] = inv[3] = 0u;
  }
}

/* bytes [0, n) of a 16-byte vector set: table of 17 masks, built once per block in LDS */
__device__ __forceinline__ void build_lowmask(u32x4_a16* lm) {
  if (threadIdx.x < 17u) {
    u32x4_a16 m;
    for (int d = 0; d < 4; d++) m[d] = bytemask(0, (int)threadIdx.x - 4 * d);
    lm[threadIdx.x] = m;
  }
}

/* o = bytes [pa, pb) from W, the rest unchanged */
__device__ __forceinline__ void merge16(u32 o[4], const u32 W[4], int pa, int pb,
                                        const u32x4_a16* lm) {
  const u32x4_a16 hi = lm[pb], lo = lm[pa];
#pragma unroll
  for (int d = 0; d < 4; d++) {
    u32 m = hi[d] & ~lo[d];
    o[d] = (o[d] & ~m) | (W[d] & m);
  }
}
__device__ __forceinline__ void merge_dash(u32 o[4], int pa, int pb, const u32x4_a16* lm) {
  const u32 dash[4] = {0x2D2D2D2Du, 0x2D2D2D2Du, 0x2D2D2D2Du, 0x2D2D2D2Du};
  merge16(o, dash, pa, pb, lm);
}

/* InvalidBase: first offender in reversed order = smallest q' index */
__device__ __forceinline__ void flag_bad_bases(const u32 inv[4], int pa, int pb, i64 S,
                                               const u32x4_a16* lm, u64* bad_base_pos) {
  const u32x4_a16 hi = lm[pb], lo = lm[pa];
  if (((inv[0] & hi[0] & ~lo[0]) | (inv[1] & hi[1] & ~lo[1]) | (inv[2] & hi[2] & ~lo[2]) |
       (inv[3] & hi[3] & ~lo[3])) == 0u)
    return;
#pragma unroll
  for (int d = 0; d < 4; d++) {
    u32 bad = inv[d] & hi[d] & ~lo[d];
    if (bad) {
      int j = 4 * d + ((__ffsll((unsigned long long)bad) - 1) >> 3);
      atomicMin(bad_base_pos, (u64)(S + j));
    }
  }
}

/* Row description shared by the emitters.  The row's events inside [c0, c0+N) are entries
 * [ga, gb) of a compacted list (G_col = tile-relative start column, G_cum = exclusive prefix of
 * gap bases — an entry's gap length is G_cum[i+1]-G_cum[i], entry gb is readable — and G_adj =
 * exclusive prefix of the source adjustment: gap bases minus skipped source bases, as wrapping
 * u32; for paf2maf rows G_adj == G_cum).  A non-gap column c reads slice index
 *     sbase + (c - c_org) - (adj before c - gcum_a)          (gcum_a = adj at c_org) */
struct RowDesc {
  u32 c_org;
  const u32* G_col;
  const u32* G_cum;
  const u32* G_adj;
  int ga, gb;
  u32 gcum_a;
  u64 sbase;
  const u32x4_a16* lowmask;
  const u32* tbl; /* granule table: T[j] = events (tile-wide index) that start before granule j */
  u32 tsh;        /* bit offset of this row's counts inside a table word */
  u32 gsh;        /* log2 of the granule width in columns (>= 4) */
  u32* queue;     /* WGA_QCAP words per wave */
};

/* generic piece walk of one chunk from an arbitrary state (any number of pieces) */
__device__ __forceinline__ void emit_walk(u32 o[4], u32 c, u32 c_end, u32 cz, int i, bool in_gap,
                                          u32 gap_end, u32 cum, const RowDesc& rd,
                                          const RowSrc& src, u64* bad_base_pos) {
  while (c < c_end) {
    if (in_gap) {
      u32 pe = gap_end < c_end ? gap_end : c_end;
      merge_dash(o, (int)(c - cz), (int)(pe - cz), rd.lowmask);
      c = pe;
      in_gap = false;
    } else {
      u32 next_gs = (i + 1 < rd.gb) ? rd.G_col[i + 1] : 0xFFFFFFFFu;
      u32 pe = next_gs < c_end ? next_gs : c_end;
      if (pe > c) {
        const int pa = (int)(c - cz), pb = (int)(pe - cz);
        const int off = (int)(cz - rd.c_org) - (int)(cum - rd.gcum_a);
        WinRaw raw;
        u32 W[4], inv[4];
        win_issue(src, rd.sbase, off, pa, pb, raw);
        win_finish(src, raw, W, inv);
        if (src.rc) flag_bad_bases(inv, pa, pb, (i64)rd.sbase + off, rd.lowmask, bad_base_pos);
        merge16(o, W, pa, pb, rd.lowmask);
        c = pe;
      }
      if (c < c_end) { /* c == start of entry i+1 */
        i++;
        u32 gs = rd.G_col[i];
        u32 gl = rd.G_cum[i + 1] - rd.G_cum[i];
        if (gl) {
          in_gap = true;
          gap_end = gs + gl;
        }
        cum = rd.G_adj[i + 1];
      }
    }
  }
}


#define WGA_TBL_SHIFT 4u                          /* granule = 16 columns */
#ifndef WGA_TBL_COLS
#define WGA_TBL_COLS 16384u /* widest tile the 16-column granule table covers (wider tiles use 32-, 64-... column granules);
                               32768 costs 4 KB more LDS and with it the sixth block per CU, and measures no faster */
#endif
#define WGA_TBL_N (WGA_TBL_COLS >> WGA_TBL_SHIFT) /* 1024 granules (+2 sentinels) */
#ifndef WGA_EMIT_U
#define WGA_EMIT_U 4 /* chunks in flight per lane */
#endif
#ifndef WGA_SOLO_BYTES
#define WGA_SOLO_BYTES 65536u /* rows up to this many bytes are emitted wave by wave, longer ones by the block */
#endif
#ifndef WGA_SPLIT_BYTES
#define WGA_SPLIT_BYTES 8192u /* ... in two halves beyond this */
#endif
#define WGA_QCAP (64u * (WGA_EMIT_U + 1u)) /* per-wave queue of complex chunks: < 64 left over + one iteration's pushes */

/* Granule table: one 16-bit field per row (target row = low half, query row = high half of a
 * word; `tsh` selects).  After the exclusive scan entry j holds, for the events of that row,
 *   bits 0-10  how many start in granules < j (tile-wide entry index of the first one at / after j)
 *   bit  11    COVER: granule j-1 begins inside a gap that started in an earlier granule
 *   bit  12    FULL:  ... and that gap runs through the end of granule j-1
 * (COVER / FULL of granule j are read from entry j+1.)  They come from +1 / -1 marks at the
 * first covered granule and after the last one; a field's prefix sums are never negative, so the
 * borrows that packed two's-complement adds take from the neighbouring fields cancel out. */
#define WGA_TBL_CNT 0x7FFu
#define WGA_TBL_COVER 0x800u
#define WGA_TBL_FULL 0x1000u
__device__ __forceinline__ void tbl_mark_event(u32* tbl, u32 gs, u32 gl, u32 gsh, u32 tsh) {
  const u32 js1 = (gs >> gsh) + 1u;
  atomicAdd(&tbl[js1 - 1u], 1u << tsh);
  const u32 ge = gs + gl;
  const u32 jc = (ge + (1u << gsh) - 1u) >> gsh, jf = ge >> gsh; /* jf <= jc */
  if (jc > js1) {
    const bool any_full = jf > js1;
    atomicAdd(&tbl[js1], (any_full ? (WGA_TBL_COVER | WGA_TBL_FULL) : WGA_TBL_COVER) << tsh);
    if (any_full && jf != jc) atomicAdd(&tbl[jf], (0u - WGA_TBL_FULL) << tsh);
    atomicAdd(&tbl[jc], (0u - ((any_full && jf == jc) ? (WGA_TBL_COVER | WGA_TBL_FULL) : WGA_TBL_COVER)) << tsh);
  }
}
/* exclusive scan of the raw per-granule marks, in place; entries [WGA_TBL_N], [WGA_TBL_N+1] = total */
__device__ __forceinline__ void tbl_scan(u32* tbl, u32* s_w4) {
  const u32 tid = threadIdx.x;
  u32 v[WGA_TBL_N / WGA_BLOCK], sum = 0;
#pragma unroll
  for (u32 e = 0; e < WGA_TBL_N / WGA_BLOCK; e++) {
    v[e] = tbl[tid * (WGA_TBL_N / WGA_BLOCK) + e];
    sum += v[e];
  }
  const u32 lane = tid & 63u, wave = WGA_WAVE_ID(tid);
  const u32 inc = wave_incl_scan_u32(sum);
  if (lane == 63u) s_w4[wave] = inc; /* callers have a barrier between the last use of s_w4 and this */
  __syncthreads();
  u32 run = inc - sum, tot = 0;
#pragma unroll
  for (u32 w = 0; w < 4; w++) {
    const u32 x = s_w4[w];
    run += w < wave ? x : 0u;
    tot += x;
  }
#pragma unroll
  for (u32 e = 0; e < WGA_TBL_N / WGA_BLOCK; e++) {
    tbl[tid * (WGA_TBL_N / WGA_BLOCK) + e] = run;
    run += v[e];
  }
  if (tid == WGA_BLOCK - 1) tbl[WGA_TBL_N] = tbl[WGA_TBL_N + 1] = tot;
}

/* Chunks are the 16-column granules of the tile-relative column space (so the granule table
 * classifies them exactly); their output address is whatever it is — stores are byte-aligned
 * 16-byte stores.  Only the first / last granule of a row span can be partial. */
struct ChunkGeom {
  u8* p;      /* address of byte 0 of the granule (may lie before the row for a head granule) */
  u32 a0, b0; /* valid bytes [a0, b0) of the 16 */
  u32 cz;     /* column of byte 0 */
  u32 c, c_end;
};
struct RowGeom {
  u8* base;    /* address of column 16*j0 */
  u32 j0;      /* first granule */
  u32 head;    /* c0 & 15 */
  u32 nchunks; /* granules touched by [c0, c0+N) */
  u32 last_b0; /* valid end of the last granule (1..16) */
};
__device__ __forceinline__ RowGeom row_geom(u8* dst, u32 N, u32 c0) {
  RowGeom r;
  r.head = c0 & 15u;
  r.j0 = c0 >> 4;
  r.base = dst - r.head; /* pointer arithmetic: stores stay global_store */
  r.nchunks = (r.head + N + 15u) >> 4;
  r.last_b0 = ((r.head + N - 1u) & 15u) + 1u;
  return r;
}
__device__ __forceinline__ ChunkGeom chunk_geom(const RowGeom& r, u32 rel) {
  ChunkGeom g;
  g.p = r.base + (rel << 4);
  g.a0 = rel == 0u ? r.head : 0u;
  g.b0 = rel == r.nchunks - 1u ? r.last_b0 : 16u;
  g.cz = (r.j0 + rel) << 4;
  g.c = g.cz + g.a0;
  g.c_end = g.cz + g.b0;
  return g;
}
__device__ __forceinline__ void chunk_store(const ChunkGeom& g, const u32 o[4]) {
  if (g.a0 == 0u && g.b0 == 16u) {
    u32x4_a1 v = {o[0], o[1], o[2], o[3]};
    *(u32x4_a1*)g.p = v;
  } else { /* partial chunk at a row / tile edge: byte stores, never read-modify-write */
    u8* p = g.p;
    for (u32 j = g.a0; j < g.b0; j++) {
      u32 d = j >> 2;
      u32 word = d == 0 ? o[0] : d == 1 ? o[1] : d == 2 ? o[2] : o[3];
      p[j] = (u8)(word >> (8u * (j & 3u)));
    }
  }
}

/* i = last entry in [ga, gb) whose column is <= c, or ga-1: two table reads and a walk over the
 * entries of one granule (0..1 entries when the granule is 16 columns wide). */
__device__ __forceinline__ int find_entry(const RowDesc& rd, u32 c) {
  const int ga = rd.ga, gb = rd.gb;
  const u32 j = c >> rd.gsh;
  int k = (int)((rd.tbl[j] >> rd.tsh) & WGA_TBL_CNT);
  const int hi = (int)((rd.tbl[j + 1] >> rd.tsh) & WGA_TBL_CNT);
  while (k < hi && rd.G_col[k] <= c) k++;
  k -= 1;
  return k < ga ? ga - 1 : (k >= gb ? gb - 1 : k);
}

/* A chunk that touches an event boundary, straight-line for rows whose windows need no bounds
 * checks:  [gap0 rest] copy0 | gap1 | copy1  with two source windows, assembled with byte masks
 * from the low-mask table; a third event inside the 16 columns continues in emit_walk.  Every
 * lane of a drain runs the same instructions whatever its chunk looks like (pieces may be
 * empty): the drains mix all shapes, so branches would only add their overhead. */
__device__ __forceinline__ u32 bfi32(u32 mask, u32 a, u32 b) { return (a & mask) | (b & ~mask); }

/* the two buffers of a row (see emit_row): source windows, biased so that small negative and
 * downward (rc) offsets stay positive, and the row's output granules */
struct RowBufs {
  BufRsrc lbuf, sbuf;
  u32 sgn, kbias;
};
__device__ __forceinline__ u32 rowbuf_loff(const RowBufs& b, int off) {
  return (((u32)off ^ b.sgn) - b.sgn) + b.kbias;
}

__device__ __forceinline__ void complex_chunk(const ChunkGeom& g, u32 rel, const RowDesc& rd,
                                              const RowSrc& src, const RowBufs& rb,
                                              u64* bad_base_pos) {
  const int ga = rd.ga, gb = rd.gb;
  const u32 c = g.c, c_end = g.c_end, cz = g.cz;
  const int i = find_entry(rd, c);
  const bool has0 = i >= ga;
  const int ic = has0 ? i : ga; /* always a readable index */
  const u32 gs0 = rd.G_col[ic], cum0a = rd.G_cum[ic], cum0b = rd.G_cum[ic + 1];
  const u32 adj0b = rd.G_adj[ic + 1];
  const u32 gl0 = cum0b - cum0a;
  const bool in_gap0 = has0 && (c - gs0 < gl0);
  const u32 adj0 = has0 ? adj0b : rd.gcum_a;
  const int n1 = i + 1;
  const u32 gs1 = n1 < gb ? rd.G_col[n1] : 0xFFFFFFFFu;
  const u32 gl1 = rd.G_cum[n1 + 1] - rd.G_cum[n1]; /* two sentinels: readable up to gb + 1 */
  const u32 adj1 = rd.G_adj[n1 + 1];
  const u32 gs2 = n1 + 1 < gb ? rd.G_col[n1 + 1] : 0xFFFFFFFFu;
  const bool hasB = gs1 < c_end;
  const u32 g0e = gs0 + gl0;
  const u32 a1 = in_gap0 ? (g0e < c_end ? g0e : c_end) : c;       /* copy piece 0 = [a1, b1) */
  const u32 b1 = hasB ? gs1 : c_end;
  const u32 g1e = gs1 + gl1;
  const u32 e1 = hasB ? (g1e < c_end ? g1e : c_end) : c_end;      /* gap 1 = [b1, e1)        */
  const u32 b2 = hasB ? (gs2 < c_end ? gs2 : c_end) : c_end;      /* copy piece 1 = [e1, b2) */
  const int offz = (int)(cz - rd.c_org);
  const int off0 = offz - (int)(adj0 - rd.gcum_a), off1 = offz - (int)(adj1 - rd.gcum_a);
  u32 o[4];
  if (src.safe) {
    WinRaw r0, r1;
    buf_load16(rb.lbuf, b1 > a1 ? rowbuf_loff(rb, off0) : WGA_BUF_OOB, r0.v);
    buf_load16(rb.lbuf, b2 > e1 ? rowbuf_loff(rb, off1) : WGA_BUF_OOB, r1.v);
    const u32x4_a16 La1 = rd.lowmask[a1 - cz], Lb1 = rd.lowmask[b1 - cz], Le1 = rd.lowmask[e1 - cz],
                    Lb2 = rd.lowmask[b2 - cz];
    u32 W0[4], W1[4], inv0[4], inv1[4];
    win_finish(src, r0, W0, inv0);
    win_finish(src, r1, W1, inv1);
    u32 bad = 0u;
#pragma unroll
    for (int d = 0; d < 4; d++) {
      const u32 m0 = Lb1[d] & ~La1[d], m1 = Lb2[d] & ~Le1[d];
      const u32 md = bfi32(Lb1[d], La1[d], Le1[d]); /* [0, a1) + [b1, e1): bytes below c are never stored */
      o[d] = bfi32(m0, W0[d], bfi32(m1, W1[d], md & 0x2D2D2D2Du));
      bad |= (inv0[d] & m0) | (inv1[d] & m1);
    }
    if (bad) { /* rare: report the first invalid base (utils.rs:97) */
      flag_bad_bases(inv0, (int)(a1 - cz), (int)(b1 - cz), (i64)rd.sbase + off0, rd.lowmask, bad_base_pos);
      flag_bad_bases(inv1, (int)(e1 - cz), (int)(b2 - cz), (i64)rd.sbase + off1, rd.lowmask, bad_base_pos);
    }
    if (b2 < c_end) /* a third event inside 16 columns: rare, generic walk from there */
      emit_walk(o, b2, c_end, cz, n1, false, 0u, adj1, rd, src, bad_base_pos);
  } else { /* a row at a pool edge: guarded byte loads, generic walk */
    o[0] = o[1] = o[2] = o[3] = 0u;
    emit_walk(o, c, c_end, cz, i, in_gap0, g0e, adj0, rd, src, bad_base_pos);
  }
  const bool whole = g.a0 == 0u && g.b0 == 16u;
  buf_store16(rb.sbuf, whole ? rel << 4 : WGA_BUF_OOB, o);
  if (!whole) chunk_store(g, o); /* a row / tile edge: byte stores */
}


/* RC = the row is read reverse-complemented: a compile-time copy of src.rc, so that each of the
 * two instantiations carries only its own window post-processing */
template <bool RC>
__device__ __forceinline__ void emit_row_t(u8* dst, u32 N, u32 c0, const RowDesc& rd,
                                           const RowSrc& src_in, u32 tid, u32 nthreads,
                                           u64* bad_base_pos) {
  if (N == 0) return;
  RowSrc src = src_in;
  src.rc = RC;
  const u32 lane = tid & 63u;
  const RowGeom rg = row_geom(dst, N, c0);
  u32* const queue = rd.queue + WGA_WAVE_ID(threadIdx.x) * WGA_QCAP; /* the wave's own, whoever it works with */
  u32 qn = 0; /* wave-uniform queue length */
  const u32 per_it = nthreads * WGA_EMIT_U;
  const u32 niter = (rg.nchunks + per_it - 1) / per_it;
  /* chunks [lo_full, lo_full + n_full) are whole 16-column granules */
  const u32 lo_full = rg.head == 0u ? 0u : 1u;
  const u32 n_full = rg.nchunks - lo_full - (rg.last_b0 == 16u ? 0u : 1u); /* may wrap to "none" */
  const bool any_full = rg.nchunks >= lo_full + (rg.last_b0 == 16u ? 0u : 1u) + 1u;
  const int koff = (int)(rd.gcum_a - rd.c_org); /* window offset of a chunk = cz + koff - adj */
  const bool row_fast = src.safe;
  const bool fast_ok = row_fast && any_full;
  /* buffers of the fast path: the source windows of this row relative to its first window (for
   * rc the windows walk down from it: offsets are biased by 2^31), and the row's output granules */
  RowBufs rb;
  rb.sgn = src.rc ? 0xFFFFFFFFu : 0u;
  rb.kbias = src.rc ? 0x80000000u : 64u;
  rb.lbuf = buf_make(src.win_base - (i64)rb.kbias, 0xFFFFFFF0u);
  rb.sbuf = buf_make(rg.base, rg.nchunks << 4);
#pragma nounroll
  for (u32 it = 0; it < niter; it++) {
    /* Fast path: a whole granule that no event of this row touches — plain copy — or that lies
     * inside one gap — dashes — read off the granule table (two words) plus one adjustment.
     * WGA_EMIT_U chunks per lane go through it together (lookups, then loads, then stores), all
     * of it branch-free: lanes without a candidate use an out-of-range buffer offset.
     * Everything else is deferred to the queue. */
    u32 rel[WGA_EMIT_U], loff[WGA_EMIT_U];
    bool act[WGA_EMIT_U], cand[WGA_EMIT_U], dash[WGA_EMIT_U];
    u32 raw[WGA_EMIT_U][4];
#pragma unroll
    for (int u = 0; u < WGA_EMIT_U; u++) {
      rel[u] = (it * WGA_EMIT_U + (u32)u) * nthreads + tid;
      act[u] = rel[u] < rg.nchunks;
      const u32 relc = act[u] ? rel[u] : 0u;
      const u32 cz = (rg.j0 + relc) << 4;
      const u32 jg = cz >> rd.gsh;
      u32 w0 = rd.tbl[jg] >> rd.tsh, w1 = rd.tbl[jg + 1] >> rd.tsh;
      WGA_PIN(w0);
      WGA_PIN(w1);
      u32 adj = rd.G_adj[w0 & WGA_TBL_CNT];
      WGA_PIN(adj);
      const u32 st = w1 & (WGA_TBL_COVER | WGA_TBL_FULL);
      dash[u] = st == (WGA_TBL_COVER | WGA_TBL_FULL);
      /* bitwise, not &&: short-circuit evaluation would come back as exec-mask branches */
      cand[u] = (bool)((int)fast_ok & (int)(rel[u] - lo_full < n_full) & (int)(((w0 ^ w1) & WGA_TBL_CNT) == 0u) &
                       (int)(st != WGA_TBL_COVER));
      const u32 off = cz + (u32)koff - adj; /* slice index of the granule relative to sbase, >= 0 */
      loff[u] = ((int)cand[u] & (int)!dash[u]) ? rowbuf_loff(rb, (int)off) : WGA_BUF_OOB;
    }
#pragma unroll
    for (int u = 0; u < WGA_EMIT_U; u++) buf_load16(rb.lbuf, loff[u], raw[u]);
    bool cxs[WGA_EMIT_U];
#pragma unroll
    for (int u = 0; u < WGA_EMIT_U; u++) {
      u32 o[4], inv[4];
      WinRaw wr;
      wr.v[0] = raw[u][0];
      wr.v[1] = raw[u][1];
      wr.v[2] = raw[u][2];
      wr.v[3] = raw[u][3];
      win_finish(src, wr, o, inv);
      const bool bad = ((inv[0] | inv[1] | inv[2] | inv[3]) != 0u) && !dash[u];
#pragma unroll
      for (int d = 0; d < 4; d++) o[d] = dash[u] ? 0x2D2D2D2Du : o[d];
      const bool st_ok = cand[u] && !bad; /* an invalid base: the complex path finds and reports it */
        buf_store16(rb.sbuf, st_ok ? rel[u] << 4 : WGA_BUF_OOB, o);
      cxs[u] = act[u] && !st_ok;
    }
    /* compact the complex chunks into the wave queue */
#pragma unroll
    for (int u = 0; u < WGA_EMIT_U; u++) {
      const u64 m = __ballot(cxs[u]);
      if (m) {
        if (cxs[u]) queue[qn + lane_rank(m, lane)] = rel[u];
        qn += (u32)__popcll(m);
      }
    }
    WGA_WAVE_SYNC();
    /* drain the queue 64 chunks at a time, and whatever is left when the row ends */
    const bool last = it + 1 >= niter;
    while (qn >= src.drain_min || (last && qn > 0u)) {
      const u32 take = qn < 64u ? qn : 64u;
      qn -= take;
      if (lane < take) {
        const u32 qrel = queue[qn + lane];
        complex_chunk(chunk_geom(rg, qrel), qrel, rd, src, rb, bad_base_pos);
      }
      WGA_WAVE_SYNC(); /* the drained slots are rewritten by the next pushes */
    }
  }
}

__device__ __forceinline__ void emit_row(u8* dst, u32 N, u32 c0, const RowDesc& rd,
                                         const RowSrc& src, u32 tid, u32 nthreads,
                                         u64* bad_base_pos) {
  if (src.rc)
    emit_row_t<true>(dst, N, c0, rd, src, tid, nthreads, bad_base_pos);
  else
    emit_row_t<false>(dst, N, c0, rd, src, tid, nthreads, bad_base_pos);
}

/* finish a RowSrc: the wave-uniform 64-bit part of every window address of this row */
__device__ __forceinline__ void rowsrc_prepare(RowSrc& s, u64 sbase) {
  s.safe = s.src_off >= 16 && s.src_off + s.src_len + 16 <= s.fa_bytes;
  s.win_base = s.rc ? s.fa + s.src_off + s.src_len - 16 - sbase : s.fa + s.src_off + sbase;
}

/* tail of a row when the fetched slice is longer than the CIGAR consumes: plain copy.  `zero2`
 * = two zero words in LDS (an empty granule table), `dummy` = any readable LDS array. */
__device__ __forceinline__ void emit_tail(u8* dst, u64 n, u64 sbase, RowSrc src,
                                          const u32x4_a16* lowmask, u32* queue, const u32* zero2,
                                          const u32* dummy, u32 tid, u32 nthreads,
                                          u64* bad_base_pos) {
  u64 done = 0;
  while (done < n) {
    u64 m = n - done;
    if (m > (1ull << 30)) m = 1ull << 30;
    RowDesc rd;
    rd.c_org = 0u;
    rd.G_col = rd.G_cum = dummy;
    rd.G_adj = zero2; /* the fast path reads G_adj[0] */
    rd.ga = rd.gb = 0;
    rd.gcum_a = 0u;
    rd.sbase = sbase + done;
    rd.lowmask = lowmask;
    rd.tbl = zero2;
    rd.tsh = 0u;
    rd.gsh = 31u;
    rd.queue = queue;
    rowsrc_prepare(src, rd.sbase);
    emit_row(dst + done, (u32)m, 0u, rd, src, tid, nthreads, bad_base_pos);
    done += m;
  }
}

/* one source byte of a row (slow path / tails): slice index -> byte, with rc + validation */
__device__ __forceinline__ u8 src_byte(const RowSrc& src, u64 sidx, u64* bad_base_pos) {
  if (sidx >= src.src_len) return (u8)'?'; /* only reachable for records flagged as panic */
  u64 raw = src.rc ? src.src_len - 1 - sidx : sidx;
  u64 idx = src.src_off + raw;
  u8 c = idx < src.fa_bytes ? src.fa[idx] : (u8)0;
  if (!src.rc) return c;
  u8 o;
  switch (c) {
    case 'A': o = 'T'; break;
    case 'C': o = 'G'; break;
    case 'G': o = 'C'; break;
    case 'T': o = 'A'; break;
    case 'N': o = 'N'; break;
    case 'a': o = 't'; break;
    case 'c': o = 'g'; break;
    case 'g': o = 'c'; break;
    case 't': o = 'a'; break;
    case 'n': o = 'n'; break;
    default:
      o = c;
      atomicMin(bad_base_pos, sidx);
  }
  return o;
}

#ifndef WGA_K2_BLOCKS
#define WGA_K2_BLOCKS 6 /* blocks per CU the register budget of k_paf2maf_expand is sized for: 80 VGPRs, no scratch,
                           26 KB of LDS.  Five (93 VGPRs, 30 KB with the 32768-column table): 7.24-7.6 ms, six: 6.88 ms */
#endif
__device__ __forceinline__ void expand_tile_v1(const ExpandArgs& a, const u64 g) {
  __shared__ u32 s_bnd[3][2];            /* (column, I | D << 16 gap-op counts) before the op where a record
                                            ends inside the tile: [0] the first such op (written in phase A),
                                            [1], [2] later ones (rebuilt on demand)               */
  __shared__ u32 s_tot[2];               /* ... and at the end of the tile                    */
  __shared__ u32 s_tg_col[WGA_TILE + 2]; /* target-row gaps (I ops): start column             */
  __shared__ u32 s_tg_cum[WGA_TILE + 2]; /*                           gap bases before        */
  __shared__ u32 s_qg_col[WGA_TILE + 2]; /* query-row gaps (D ops)                            */
  __shared__ u32 s_qg_cum[WGA_TILE + 2];
  __shared__ u32 s_zero2[2];
  __shared__ u32 s_w4[16];
  __shared__ u32x4_a16 s_lowmask[17];
  __shared__ u32 s_tbl[WGA_TBL_N + 2];   /* entries before each 16-column granule: I | D<<16  */
  __shared__ u32 s_queue[4 * WGA_QCAP];  /* per-wave queues of complex chunks                 */

  const u32 tid = threadIdx.x;
  const u32 lane = tid & 63u, wave = WGA_WAVE_ID(tid);
  const u64 tile_start = g * WGA_TILE;
  const u64 tile_end = tile_start + WGA_TILE < a.n_ops ? tile_start + WGA_TILE : a.n_ops;
  const u32 nt = (u32)(tile_end - tile_start);
  build_lowmask(s_lowmask);
  /* lane k of every wave holds dword k of this tile's wga_tile_desc: one VGPR, no dependent
   * loads; fields are picked out with v_readlane when they are needed */
  u32 pre = 0u;
  if (lane < 32u) pre = ((const u32*)(a.tdesc + g))[lane];
  const u64 tile_cols = wave_get_u64(pre, 0);
  const bool fast = !a.force_slow && tile_cols <= WGA_FAST_COL_LIMIT;
  /* granule width: 16 columns unless the tile is wider than the table covers */
  u32 gsh = a.no_table ? 8u : WGA_TBL_SHIFT;
  while ((tile_cols >> gsh) >= WGA_TBL_N) gsh++;
  const bool use_tbl = fast;
  const u32 r0 = wave_get_u32(pre, 2);
  /* op index (tile-relative) where the tile's first record ends; >= nt if it does not end here */
  const u64 re0 = wave_get_u64(pre, 12);
  const u32 kb0 = re0 < tile_end ? (u32)(re0 - tile_start) : 0xFFFFFFFFu;
  if (use_tbl)
    for (u32 k = tid; k < WGA_TBL_N + 2u; k += WGA_BLOCK) s_tbl[k] = 0u;
  if (tid < 2u) s_zero2[tid] = 0u;

  /* ---- phase A: 4 consecutive ops per thread, block scan into LDS -------------------------- */
  u32 opw[4];
  {
    u32 base = tid * 4u;
    if (base + 3 < nt) {
      u32x4_a16 v = ops_load16(a.ops + tile_start + base);
      opw[0] = v[0];
      opw[1] = v[1];
      opw[2] = v[2];
      opw[3] = v[3];
    } else {
      for (int e = 0; e < 4; e++) opw[e] = (base + e < nt) ? a.ops[tile_start + base + e] : 0u;
    }
  }
  /* exclusive (column, gap-op counts) prefix at this thread's first op, kept for record boundaries
   * beyond the first one (per-op prefix arrays would cost 8 KB of LDS and the fifth block per CU) */
  u32 my_col = 0, my_cnt = 0;
  if (fast) {
    u32 cls[4];
    u32 l[4], sl = 0, si = 0, sd = 0, cnt = 0;
    for (int e = 0; e < 4; e++) {
      u32 code = opw[e] & 15u, len = opw[e] >> 4;
      cls[e] = op_class(code);
      l[e] = (cls[e] <= CLS_D) ? len : 0u;
      sl += l[e];
      si += cls[e] == CLS_I ? len : 0u;
      sd += cls[e] == CLS_D ? len : 0u;
      cnt += cls[e] == CLS_I ? 1u : (cls[e] == CLS_D ? 0x10000u : 0u);
    }
    /* exclusive prefixes of (columns, I bases, D bases, gap-op counts): every component stays
     * below 2^31 on the fast path */
    const u32 sv[4] = {sl, si, sd, cnt};
    u32 sx[4], stot[4];
    block_excl_scan4_u32(sv, sx, stot, s_w4, true);
    u32 x_col = sx[0], x_i = sx[1], x_d = sx[2], x_cnt = sx[3];
    my_col = x_col;
    my_cnt = x_cnt;
    for (int e = 0; e < 4; e++) {
      if (tid * 4u + (u32)e == kb0) { /* the tile's first record ends before this op */
        s_bnd[0][0] = x_col;
        s_bnd[0][1] = x_cnt;
      }
      const bool isi = cls[e] == CLS_I, isd = cls[e] == CLS_D;
      if (isi | isd) { /* ONE instance for both kinds of gap op: the body runs once per wave and op slot */
        const u32 len = opw[e] >> 4;
        const u32 slot = isi ? (x_cnt & 0xFFFFu) : (x_cnt >> 16);
        u32* const g_col = isi ? s_tg_col : s_qg_col;
        u32* const g_cum = isi ? s_tg_cum : s_qg_cum;
        g_col[slot] = x_col;
        g_cum[slot] = isi ? x_i : x_d;
        if (use_tbl) tbl_mark_event(s_tbl, x_col, len, gsh, isi ? 0u : 16u);
        x_i += isi ? len : 0u;
        x_d += isi ? 0u : len;
        x_cnt += isi ? 1u : 0x10000u;
      }
      x_col += l[e];
    }
    if (tid == WGA_BLOCK - 1) { /* sentinels: totals (two, so that index i+1 is always readable) */
      s_tot[0] = x_col;
      s_tot[1] = x_cnt;
      s_tg_col[x_cnt & 0xFFFFu] = x_col;
      s_tg_cum[x_cnt & 0xFFFFu] = x_i;
      s_tg_col[(x_cnt & 0xFFFFu) + 1u] = x_col;
      s_tg_cum[(x_cnt & 0xFFFFu) + 1u] = x_i;
      s_qg_col[x_cnt >> 16] = x_col;
      s_qg_cum[x_cnt >> 16] = x_d;
      s_qg_col[(x_cnt >> 16) + 1u] = x_col;
      s_qg_cum[(x_cnt >> 16) + 1u] = x_d;
    }
    if (use_tbl) { /* raw marks -> exclusive prefix */
      __syncthreads();
      tbl_scan(s_tbl, s_w4);
    }
  }
  __syncthreads();

  /* ---- phase B: walk the record segments of this tile ------------------------------------- */
  u32 r = r0;
  u64 cur = tile_start;
  u64 re = wave_get_u64(pre, 12);
  u32 bnd_col = 0u, bnd_ev = 0u, nseg = 0u; /* prefix at the start of the current segment */
  while (cur < tile_end) {
    while (re <= cur) {
      r++;
      re = a.op_off[r + 1];
    }
    const bool is0 = r == r0;
    const u64 rs = is0 ? wave_get_u64(pre, 10) : a.op_off[r];
    const u64 seg_end = re < tile_end ? re : tile_end;
    const u32 kb = (u32)(seg_end - tile_start);

    /* class sums of this record before the tile (only the tile's first segment can continue a
     * record; k_tile_base worked them out) and the record's geometry (k_rec_desc) */
    u64 b_mx = 0, b_i = 0, b_d = 0;
    if (rs < tile_start) { /* only the tile's first record can continue from earlier tiles */
      b_mx = wave_get_u64(pre, 4);
      b_i = wave_get_u64(pre, 6);
      b_d = wave_get_u64(pre, 8);
    }
    const u64 cb = b_mx + b_i + b_d; /* record-relative column of the segment start */
    const u64 tb = b_mx + b_d;       /* target bases consumed before it              */
    const u64 qb = b_mx + b_i;       /* query bases consumed before it               */

    /* The record's geometry stays spread over the lanes of `dsc` (layout of wga_tile_desc lanes
     * 14..31, strand in lane 3): a field costs one v_readlane where it is used instead of an
     * SGPR pair held — and spilled — across the whole segment. */
    u32 dsc = pre;
    if (!is0) {
      const u32* rp = (const u32*)(a.recs + r);
      dsc = 0u;
      if (lane >= 14u && lane < 32u) dsc = rp[lane - 14u];
      if (lane == 3u) dsc = rp[18];
    }
    const u64 t_src_len = wave_get_u64(dsc, 20), q_src_len = wave_get_u64(dsc, 24);
    u64* const bad_base = (u64*)&a.diag[r].bad_base_pos;
    u64* const panic_idx = (u64*)&a.diag[r].panic_op_idx;

    u32 col_a = 0, seg_cols = 0, icum_a = 0, dcum_a = 0;
    int ia = 0, ib = 0, ja = 0, jb = 0;
    if (fast) {
      u32 col_b, evb;
      if (kb == nt) {
        col_b = WGA_UNI32(s_tot[0]);
        evb = WGA_UNI32(s_tot[1]);
      } else if (nseg == 0u) { /* written in phase A */
        col_b = WGA_UNI32(s_bnd[0][0]);
        evb = WGA_UNI32(s_bnd[0][1]);
      } else { /* a further record ends inside the tile: the owner of op kb rebuilds its prefix */
        u32* const slot = s_bnd[1u + (nseg & 1u)];
        if (tid == (kb >> 2)) {
          u32 c = my_col, n = my_cnt;
          for (u32 e = 0; e < (kb & 3u); e++) {
            const u32 op = a.ops[tile_start + (kb & ~3u) + e];
            const u32 cl = op_class(op & 15u);
            c += cl <= CLS_D ? (op >> 4) : 0u;
            n += cl == CLS_I ? 1u : (cl == CLS_D ? 0x10000u : 0u);
          }
          slot[0] = c;
          slot[1] = n;
        }
        __syncthreads(); /* uniform: every thread walks the same segments */
        col_b = WGA_UNI32(slot[0]);
        evb = WGA_UNI32(slot[1]);
      }
      col_a = bnd_col;
      seg_cols = col_b - col_a;
      const u32 eva = bnd_ev;
      bnd_col = col_b;
      bnd_ev = evb;
      ia = (int)(eva & 0xFFFFu);
      ib = (int)(evb & 0xFFFFu);
      ja = (int)(eva >> 16);
      jb = (int)(evb >> 16);
      icum_a = WGA_UNI32(s_tg_cum[ia]);
      dcum_a = WGA_UNI32(s_qg_cum[ja]);

      /* String::insert_str panics when the insertion point is beyond the string
       * (cigar.rs:507,513): an I (D) op whose target (query) consumption so far exceeds the
       * fetched slice.  Checked on the compact gap lists; the exact op index is only worked out
       * (serial rescan by the detecting thread) when that ever happens. */
      bool pan = false;
      for (int i = ia + (int)tid; i < ib; i += (int)WGA_BLOCK)
        pan |= tb + (u64)(s_tg_col[i] - col_a) - (u64)(s_tg_cum[i] - icum_a) > t_src_len;
      for (int i = ja + (int)tid; i < jb; i += (int)WGA_BLOCK)
        pan |= qb + (u64)(s_qg_col[i] - col_a) - (u64)(s_qg_cum[i] - dcum_a) > q_src_len;
      if (pan) {
        u64 tp = tb, qp = qb;
        for (u64 k = cur; k < seg_end; k++) {
          const u32 op = a.ops[k];
          const u32 c = op_class(op & 15u);
          const u64 len = op >> 4;
          if ((c == CLS_I && tp > t_src_len) || (c == CLS_D && qp > q_src_len)) {
            atomicMin(panic_idx, k - rs);
            break;
          }
          if (c == CLS_MX || c == CLS_D) tp += len;
          if (c == CLS_MX || c == CLS_I) qp += len;
        }
      }
    } else {
      /* u64 fallback for tiles wider than 2^31 columns: ops are walked serially (every thread
       * redundantly), each op's columns are written block-strided, one byte per store */
      RowSrc ts, qs;
      ts.fa = a.t_fa;
      ts.fa_bytes = a.t_fa_bytes;
      ts.src_off = wave_get_u64(dsc, 18);
      ts.src_len = t_src_len;
      ts.rc = false;
      qs.fa = a.q_fa;
      qs.fa_bytes = a.q_fa_bytes;
      qs.src_off = wave_get_u64(dsc, 22);
      qs.src_len = q_src_len;
      qs.rc = (wave_get_u32(dsc, 3) & 1u) != 0u;
      const u64 t_row_len = t_src_len + wave_get_u64(dsc, 26), q_row_len = q_src_len + wave_get_u64(dsc, 28);
      u8* const t_dst = a.out + wave_get_u64(dsc, 14);
      u8* const q_dst = a.out + wave_get_u64(dsc, 16);
      u64 x = cb, tp = tb, qp = qb;
      for (u64 k = cur; k < seg_end; k++) {
        const u32 op = a.ops[k];
        const u32 c = op_class(op & 15u);
        const u64 len = op >> 4;
        if (c == CLS_I && tp > ts.src_len && tid == 0) atomicMin(panic_idx, k - rs);
        if (c == CLS_D && qp > qs.src_len && tid == 0) atomicMin(panic_idx, k - rs);
        if (c <= CLS_D) {
          for (u64 j = tid; j < len; j += WGA_BLOCK) {
            if (x + j < t_row_len) t_dst[x + j] = (c == CLS_I) ? (u8)'-' : src_byte(ts, tp + j, bad_base);
            if (x + j < q_row_len) q_dst[x + j] = (c == CLS_D) ? (u8)'-' : src_byte(qs, qp + j, bad_base);
          }
          x += len;
          if (c != CLS_I) tp += len;
          if (c != CLS_D) qp += len;
        }
      }
    }

    /* Row jobs through ONE emit_row site (keeps the kernel small enough for the I-cache):
     * 0/1 = this segment of the target / query row (rows end where a short slice ends);
     * 2/3 = once the record ends in this tile, what the slices hold beyond the CIGAR. */
    const bool rec_ends = seg_end == re;
    const u32 rec_flags = wave_get_u32(dsc, 3);
#pragma nounroll
    for (int job = 0; job < 4; job++) {
      const bool is_q = (job & 1) != 0, is_tail = job >= 2;
      if (is_tail && (!rec_ends || !(rec_flags & (is_q ? 4u : 2u)))) continue; /* no tail: nothing read, nothing computed */
      /* Ownership is static: piece p of this job goes to wave (job + 2 p + segment index) mod 4 — the two halves of
       * the two rows of a segment land on four different waves, and the rotation with the segment spreads the
       * single-piece rows of short records.  A wave that owns neither piece reads nothing of the job (rows beyond
       * WGA_SOLO_BYTES are the whole block's: only possible when the segment is that wide). */
#ifndef WGA_OWN_STRIDE
#define WGA_OWN_STRIDE 2u /* piece 1 of a job goes to the wave this many behind piece 0's */
#endif
      const u32 own0 = ((u32)job * (WGA_OWN_STRIDE == 2u ? 1u : 2u) + nseg) & 3u, own1 = (own0 + WGA_OWN_STRIDE) & 3u;
      if (!is_tail && seg_cols <= WGA_SOLO_BYTES && own0 != wave && own1 != wave) continue;
      /* this row's fields: the query ones sit 2 (offsets, gap totals) or 4 (slice) lanes after
       * the target ones. */
      const int q2 = is_q ? 2 : 0, q4 = is_q ? 4 : 0;
      const u64 gap_total = wave_get_u64(dsc, 26 + q2); /* I bases (target row) / D bases (query row) */
      const u64 L = wave_get_u64(dsc, 30);
      const u64 src_len = is_q ? q_src_len : t_src_len;
      const u64 row_len = src_len + gap_total;
      u64 x0, nbytes;
      if (!is_tail) {
        if (!fast) continue;
        const u64 x1 = cb + seg_cols < row_len ? cb + seg_cols : row_len;
        x0 = cb;
        nbytes = x1 > cb ? x1 - cb : 0;
      } else {
        if (!rec_ends) continue;
        x0 = L;
        nbytes = row_len > L ? row_len - L : 0;
      }
      if (nbytes == 0) continue;
      /* Rows of ordinary size are not shared out thread by thread: a row (or each half of it, cut
       * on a granule boundary) is taken by ONE wave, round-robin over the tile's row jobs — one
       * prologue and one set of queue drains per row instead of four quarter-full ones.  Only
       * rows beyond WGA_SOLO_BYTES (giant tiles) are emitted by the whole block together. */
      const bool coop = nbytes > WGA_SOLO_BYTES;
      const u32 c_row = is_tail ? 0u : col_a; /* column of the row's first byte */
      u64 cut = nbytes;                        /* first piece = [0, cut), second = [cut, nbytes) */
      if (!coop && nbytes > WGA_SPLIT_BYTES) {
        const u32 cc = (c_row + (u32)(nbytes >> 1)) & ~15u;
        if (cc > c_row && (u64)(cc - c_row) < nbytes) cut = cc - c_row;
      }
      for (int piece = 0; piece < 2; piece++) {
        const u64 lo = piece == 0 ? 0 : cut, hi = piece == 0 ? cut : nbytes;
        if (lo >= hi) continue;
        if (!coop && (piece == 0 ? own0 : own1) != wave) continue;
        /* only the wave that owns a row piece reads the row's source / destination fields */
        RowSrc src;
        src.fa = is_q ? a.q_fa : a.t_fa;
        src.fa_bytes = is_q ? a.q_fa_bytes : a.t_fa_bytes;
        src.src_off = wave_get_u64(dsc, 18 + q4);
        src.src_len = src_len;
        src.rc = is_q && (wave_get_u32(dsc, 3) & 1u) != 0u;
        src.drain_min = a.drain_min;
        u8* const dst = a.out + wave_get_u64(dsc, 14 + q2) + x0;
        const u64 sb0 = is_tail ? L - gap_total : (is_q ? qb : tb);
        for (u64 done = lo; done < hi; done += (1ull << 30)) {
          const u64 m = hi - done < (1ull << 30) ? hi - done : (1ull << 30);
          RowDesc rd;
          rd.c_org = is_tail ? 0u : col_a;
          rd.G_col = is_q ? s_qg_col : s_tg_col;
          rd.G_cum = is_q ? s_qg_cum : s_tg_cum;
          rd.G_adj = is_tail ? s_zero2 : rd.G_cum; /* a tail's fast path reads G_adj[0]: the gap lists are not even
                                                      initialised when the tile takes the op-serial walk */
          rd.ga = is_tail ? 0 : (is_q ? ja : ia);
          rd.gb = is_tail ? 0 : (is_q ? jb : ib);
          rd.gcum_a = is_tail ? 0u : (is_q ? dcum_a : icum_a);
          rd.sbase = is_tail ? sb0 + done : sb0;
          rd.lowmask = s_lowmask;
          rd.tbl = is_tail ? s_zero2 : s_tbl;
          rd.tsh = (is_q && !is_tail) ? 16u : 0u;
          rd.gsh = is_tail ? 31u : gsh;
          rd.queue = s_queue;
          rowsrc_prepare(src, rd.sbase);
          emit_row(dst + done, (u32)m, is_tail ? 0u : col_a + (u32)done, rd, src, coop ? tid : lane,
                   coop ? WGA_BLOCK : 64u, bad_base);
        }
      }
    }
    cur = seg_end;
    r++;
    if (cur < tile_end) re = a.op_off[r + 1];
    nseg++;
  }
}

/* v1 of the row kernel (granules stored as they are produced: lines reach the L2 in pieces): `expand_variant` 0, one block
 * per tile of the batch — and, as k_paf2maf_expand_list, the kernel of the tiles the streaming kernel (wga_kernels_k2s.h, the
 * default) leaves: records that are not clean, pool edges, tiles beyond 2^24 columns, the op-serial u64 walk beyond 2^31. */
/* Blocks go to the 8 XCDs round robin (block b runs on XCD b % 8), each with its own L2.  Every XCD gets one contiguous
 * eighth of the tiles, in order: the ~190 tiles an XCD has in flight are then neighbours — the output lines two tiles
 * share and the source windows of one record's tiles meet in one L2.  Measured (profiles/r02_k2_experiments.md):
 * 6.75 -> 6.65 ms with 2 x 50 Mb pools, 7.69 -> 6.9-7.3 ms with 2 x 1 Gb pools (against tile = block). */
__device__ __forceinline__ u64 xcd_tile_of_block() {
  const u32 nt = gridDim.x, b = blockIdx.x, x = b & 7u, q = nt >> 3, r = nt & 7u;
  return (u64)(x * q + (x < r ? x : r) + (b >> 3));
}
__global__ __launch_bounds__(256, WGA_K2_BLOCKS) void k_paf2maf_expand(ExpandArgs a) {
  expand_tile_v1(a, xcd_tile_of_block());
}

__global__ __launch_bounds__(256, 4) void k_paf2maf_expand_list(ExpandArgs a) {
  const u32 n_list = *a.tile_count;
  for (u32 idx = blockIdx.x; idx < n_list; idx += gridDim.x) {
    expand_tile_v1(a, a.tile_list[idx]);
    __syncthreads(); /* the tile's LDS state is dead */
  }
}

#endif /* WGA_K2_V1_H */
