/*
 * wga_kernels.h — the core every kernel header of the wgatools CIGAR hot path includes, and what the streaming row kernel
 * (wga_kernels_k2s.h) is compiled from besides its own file and wga_intrin.h.  Hand-written HIP for gfx950 (CDNA4, wave64);
 * integer / byte work, HBM-bound: no MFMA anywhere.
 *
 * Work decomposition (all op-stream kernels): the packed op stream of a whole batch is cut into
 * *globally aligned tiles* of WGA_TILE ops, independent of record boundaries, so the load is
 * balanced whatever the record-length skew (1-op records and 2 Mop records in one launch).  Small
 * pre-pass kernels (k_tile_rec in wga_k1_stat.h; k_rec_desc, k_tile_base here) tell every tile which record its first op
 * belongs to and where that record stands, so that the walk kernels start with one load.
 *
 * In this file:
 *   - the base types, the tile constants, the op classes and K1's tile summary (wga_tile_sum);
 *   - the wave and block reductions and scans, wga_find_rec;
 *   - the paf2maf layout step (ScanLayout, k_layout_rows);
 *   - the byte helpers both row kernels use (comp4, bswap32, alignbyte, bytemask);
 *   - the row pre-pass and its types (k_rec_desc, k_tile_base, wga_tile_desc) and the row kernels' arguments (ExpandArgs).
 * Everything else has a header of its own, one per kernel family: wga_k1_stat.h (K1), wga_scan.h (the generic scan of every
 * count -> fill launcher), wga_k2_v1.h (v1 of the row kernel), wga_kernels_k2s.h (K2s), wga_k_class.h, wga_k_peers.h,
 * wga_k3_maf.h ... wga_k28_maf2paf.h; wga_text_out.h is what the text writers among them share.
 *
 * The same source also compiles under tests/emu/simt_emu.h for CPU-side logic tests: wga_intrin.h is the one place that
 * knows (it hands its names over to tests/emu/wga_intrin_emu.h there).
 */
#ifndef WGA_KERNELS_H
#define WGA_KERNELS_H

#include "../../include/wga_hip.h"
#include "wga_rt.h"

typedef unsigned int u32;
typedef unsigned long long u64;
typedef long long i64;
typedef unsigned char u8;

#define WGA_TILE 1024u
#define WGA_BLOCK 256u
#define WGA_FAST_COL_LIMIT 0x7FFFFFFFull /* tile-relative columns kept in u32 on the fast path */

/* op classes */
#define CLS_MX 0u
#define CLS_I 1u
#define CLS_D 2u
#define CLS_S 3u
#define CLS_O 4u /* N H P OTHER: consume neither row in paf2maf terms; "move" for pafcov */

/* class of a packed op code (4 bits) — 3 bits per code packed into a 64-bit constant */
__device__ __forceinline__ u32 op_class(u32 code) {
  /* code: 0 M,1 I,2 D,3 N,4 S,5 H,6 P,7 =,8 X,9 Icont,10 Dcont,11.. other */
  const u64 lut = (u64)CLS_MX | ((u64)CLS_I << 3) | ((u64)CLS_D << 6) | ((u64)CLS_O << 9) |
                  ((u64)CLS_S << 12) | ((u64)CLS_O << 15) | ((u64)CLS_O << 18) |
                  ((u64)CLS_MX << 21) | ((u64)CLS_MX << 24) | ((u64)CLS_I << 27) |
                  ((u64)CLS_D << 30) | ((u64)CLS_O << 33) | ((u64)CLS_O << 36) |
                  ((u64)CLS_O << 39) | ((u64)CLS_O << 42) | ((u64)CLS_O << 45);
  return (u32)(lut >> (code * 3)) & 7u;
}

/* tile summary: class sums over the whole tile and over its last record segment */
struct wga_tile_sum {
  u64 tot[5];
  u64 tail[5];
  u64 rec; /* record that owns the first op of the tile (saves later kernels the search) */
};

/* a 16-byte vector that only promises dword alignment (global_load_dwordx4 needs no more) */
typedef u32 u32x4_a4 __attribute__((vector_size(16), aligned(4)));
typedef u32 u32x4_a16 __attribute__((vector_size(16), aligned(16)));
/* byte-aligned 16-byte access: one global_load/store_dwordx4 on gfx950 (unaligned loads measure
 * the same as aligned ones, unaligned stores ~10 % slower: scripts/micro/unaligned_copy.hip) */
typedef u32 u32x4_a1 __attribute__((vector_size(16), aligned(1)));

#include <type_traits>

#include "wga_intrin.h" /* the gfx950 instructions the kernels are written with (cross-lane, buffer, uniformity) */

__device__ __forceinline__ u64 wave_sum_u64(u64 v) {
  for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m);
  return v;
}
/* exact sum of 64 u32 values (up to 2^38): two 16-bit halves scanned separately */
__device__ __forceinline__ u64 wave_sum_u32_wide(u32 v) {
  const u32 lo = wave_last_u32(wave_incl_scan_u32(v & 0xFFFFu));
  const u32 hi = wave_last_u32(wave_incl_scan_u32(v >> 16));
  return ((u64)hi << 16) + (u64)lo;
}
__device__ __forceinline__ u32 wave_sum_u32(u32 v) { return wave_last_u32(wave_incl_scan_u32(v)); }
/* inclusive scan of a u64 over the 64 lanes */
__device__ __forceinline__ u64 wave_incl_scan_u64(u64 v, u32 lane) {
#pragma unroll
  for (u32 d = 1; d < 64; d <<= 1) {
    const u64 o = __shfl_up(v, d);
    if (lane >= d) v += o;
  }
  return v;
}
__device__ __forceinline__ u32 wave_min_u32(u32 v) {
  for (int m = 32; m >= 1; m >>= 1) {
    u32 o = __shfl_xor(v, m);
    v = o < v ? o : v;
  }
  return v;
}

/* exclusive scan of four u32 values across a 256-thread block; tot[] = block totals.
 * s_w4: 16 words of LDS. */
__device__ __forceinline__ void block_excl_scan4_u32(const u32 v[4], u32 ex[4], u32 tot[4],
                                                     u32* s_w4, bool s_w4_idle = false) {
  const u32 lane = threadIdx.x & 63u, wave = WGA_WAVE_ID(threadIdx.x);
  u32 inc[4];
#pragma unroll
  for (int k = 0; k < 4; k++) inc[k] = wave_incl_scan_u32(v[k]);
  if (!s_w4_idle) __syncthreads(); /* protect s_w4 reuse */
  if (lane == 63u) {
#pragma unroll
    for (int k = 0; k < 4; k++) s_w4[wave * 4 + k] = inc[k];
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < 4; k++) {
    u32 pre = 0, t = 0;
#pragma unroll
    for (u32 w = 0; w < 4; w++) {
      const u32 x = s_w4[w * 4 + k];
      pre += w < wave ? x : 0u;
      t += x;
    }
    ex[k] = pre + inc[k] - v[k];
    tot[k] = t;
  }
}

/* Last r in [0, n] with off[r] <= x (off is non-decreasing, off[0] == 0).  Wave-uniform call:
 * a 64-ary search, one coalesced probe + ballot per level. */
__device__ __forceinline__ u32 wga_find_rec(const u64* off, u32 n, u64 x) {
  u32 lane = threadIdx.x & 63u;
  u64 lo = 0, hi = (u64)n + 1;
  while (hi - lo > 1) {
    u64 span = hi - lo;
    u64 step = (span + 63) >> 6;
    u64 p = lo + (u64)(lane + 1) * step;
    int pred = (p < hi) && (off[p] <= x);
    u64 m = __ballot(pred);
    u64 k = (u64)__popcll(m);
    u64 nhi = lo + (k + 1) * step;
    lo = lo + k * step;
    hi = nhi < hi ? nhi : hi;
  }
  return (u32)lo;
}

/* exclusive scan of one u64 across a 256-thread block; *total = the block total.  s_w: 5 words of LDS. */
__device__ __forceinline__ u64 block_excl_scan_u64(u64 v, u64* s_w /*[5]*/, u64* total) {
  const u32 lane = threadIdx.x & 63u, wave = WGA_WAVE_ID(threadIdx.x);
  u64 inc = v;
  for (u32 d = 1; d < 64; d <<= 1) {
    u64 t = __shfl_up(inc, d);
    if (lane >= d) inc += t;
  }
  __syncthreads(); /* protect s_w reuse */
  if (lane == 63) s_w[wave] = inc;
  __syncthreads();
  u64 pre = 0, tot = 0;
  for (u32 k = 0; k < 4; k++) {
    u64 x = s_w[k];
    if (k < wave) pre += x;
    tot += x;
  }
  *total = tot;
  return pre + inc - v;
}

/* ============================================================================================ */
/* the paf2maf layout step                                                                      */
/* ============================================================================================ */
/* value functor of the layout's scan (wga_scan.h): bytes one record occupies in the output text */
struct ScanLayout {
  const wga_cigar_counts* counts;
  const u64* t_src_len;
  const u64* q_src_len;
  const u32* pre_t;
  const u32* pre_q;
  const u32* post;
  __device__ u64 t_row(u32 i) const { /* String::insert_str grows the target by the I bases */
    return t_src_len[i] + counts[i].ins_bp + counts[i].inv_ins_bp;
  }
  __device__ u64 q_row(u32 i) const { return q_src_len[i] + counts[i].del_bp + counts[i].inv_del_bp; }
  __device__ u64 operator()(u32 i) const {
    return (u64)(pre_t ? pre_t[i] : 0u) + t_row(i) + (u64)(pre_q ? pre_q[i] : 0u) + q_row(i) +
           (u64)(post ? post[i] : 0u);
  }
};

/* row offsets from record offsets (converter.rs:237-262 + maf.rs:566-581 geometry) */
__global__ __launch_bounds__(256) void k_layout_rows(ScanLayout f, u32 n, const u64* rec_off,
                                                     u64* t_row_off, u64* q_row_off) {
  u32 i = blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  u64 t = rec_off[i] + (f.pre_t ? f.pre_t[i] : 0u);
  u64 q = t + f.t_row(i) + (f.pre_q ? f.pre_q[i] : 0u);
  t_row_off[i] = t;
  q_row_off[i] = q;
}

/* ============================================================================================ */
/* byte helpers of the two row kernels                                                          */
/* ============================================================================================ */
/* Complement 4 packed bases (utils.rs:86-96) with two 8-entry byte LUTs indexed by the low
 * THREE bits of each base — A=1 C=3 T=4 N=6 G=7 are distinct.  `fold` is the upper-case base a
 * valid byte must equal once its case bit is cleared (0xFF for the unused indices, which no
 * byte & 0xDF can equal), `comp` its complement.  *bad gets a non-zero byte wherever the input
 * is not one of ACGTNacgtn. */
__device__ __forceinline__ u32 comp4(u32 x, u32* bad) {
  const u32 sel = x & 0x07070707u;
  /* index:      7     6     5     4        3     2     1     0   */
  const u32 fold = byte_perm(0x474EFF54u, 0x43FF41FFu, sel); /* G N - T | C - A - */
  const u32 comp = byte_perm(0x434EFF41u, 0x47FF54FFu, sel); /* C N - A | G - T - */
  *bad = (x & 0xDFDFDFDFu) ^ fold;
  return comp | (x & 0x20202020u);
}

__device__ __forceinline__ u32 bswap32(u32 x) {
  return (x >> 24) | ((x >> 8) & 0xFF00u) | ((x << 8) & 0xFF0000u) | (x << 24);
}
__device__ __forceinline__ u32 alignbyte(u32 hi, u32 lo, u32 sh) {
  return (u32)(((((u64)hi) << 32) | (u64)lo) >> (8u * sh));
}
/* bytes [lo,hi) ∩ [0,4) of a dword as a 0xFF mask */
__device__ __forceinline__ u32 bytemask(int lo, int hi) {
  lo = lo < 0 ? 0 : lo;
  hi = hi > 4 ? 4 : hi;
  if (hi <= lo) return 0u;
  u32 mh = hi >= 4 ? 0xFFFFFFFFu : ((1u << (8 * hi)) - 1u);
  u32 ml = (1u << (8 * lo)) - 1u;
  return mh & ~ml;
}

/* ============================================================================================ */
/* the row pre-pass: what a row kernel (K2s, v1, K6's rows) is told about records and tiles     */
/* ============================================================================================ */
/* Per-record geometry gathered once (k_rec_desc) so that the expand kernel fetches one compact
 * struct per segment instead of ten scattered values; per-tile base sums of the record that
 * continues into a tile (k_tile_base) so that it never walks tile summaries itself. */
struct wga_rec_desc {
  u64 t_row_off, q_row_off;
  u64 t_src_off, t_src_len, q_src_off, q_src_len;
  u64 I_total, D_total, L;
  u64 neg;
};
struct wga_tile_base {
  u64 mx, i, d;
};
/* Everything the expand kernel needs before it can start on a tile, in one 128-byte record that
 * every wave fetches with a single 32-lane load at the top of the kernel (no dependent round
 * trips: tile summary -> record index -> offsets / descriptor).  Dword layout is fixed: the
 * kernel picks fields out of lanes with v_readlane. */
struct wga_tile_desc {
  u64 tile_cols;        /* dwords 0-1   columns of the tile (M = X I D bases)                  */
  u32 rec, neg;         /* 2, 3         record of the tile's first op; its strand              */
  u64 b_mx, b_i, b_d;   /* 4-9          class sums of that record before the tile              */
  u64 rs, re;           /* 10-13        op_off[rec], op_off[rec + 1]                           */
  u64 t_row_off, q_row_off, t_src_off, t_src_len, q_src_off, q_src_len, I_total, D_total, L; /* 14-31 */
};

__global__ __launch_bounds__(256) void k_rec_desc(u32 n, const wga_cigar_counts* counts,
                                                  const u8* strand_neg, const u64* t_src_off,
                                                  const u64* t_src_len, const u64* q_src_off,
                                                  const u64* q_src_len, const u64* t_row_off,
                                                  const u64* q_row_off, wga_rec_desc* out, const u64* op_off,
                                                  u64 t_fa_bytes, u64 q_fa_bytes, u8* tile_flag) {
  u32 r = blockIdx.x * 256u + threadIdx.x;
  if (r >= n) return;
  const wga_cigar_counts cn = counts[r];
  wga_rec_desc d;
  d.t_row_off = t_row_off[r];
  d.q_row_off = q_row_off[r];
  d.t_src_off = t_src_off[r];
  d.t_src_len = t_src_len[r];
  d.q_src_off = q_src_off[r];
  d.q_src_len = q_src_len[r];
  d.I_total = cn.ins_bp + cn.inv_ins_bp;
  d.D_total = cn.del_bp + cn.inv_del_bp;
  d.L = cn.match + cn.mismatch + d.I_total + d.D_total;
  /* bit 0 strand; bits 1 / 2: the target / query slice is longer than the CIGAR consumes (a tail to append) — lets the
   * row kernels skip the two tail jobs of a record, which are empty in any consistent PAF, without reading a field */
  /* bit 3: a slice is shorter than its CIGAR consumes — the only case in which String::insert_str can be asked to insert beyond
   * the end (cigar.rs:507,513); the window kernel checks the gap lists of such records only */
  d.neg = (strand_neg[r] != 0 ? 1u : 0u) | (d.t_src_len + d.I_total > d.L ? 2u : 0u) | (d.q_src_len + d.D_total > d.L ? 4u : 0u) |
          ((d.t_src_len + d.I_total < d.L || d.q_src_len + d.D_total < d.L) ? 8u : 0u);
  out[r] = d;
  /* the streaming row kernel's pre-pass (tile_flag != NULL; wga_kernels_k2s.h): a record that is not clean (flags 2 / 4 / 8), or
   * whose slices lie within 32 bytes of an edge of their pool (that kernel's sixteen-byte windows reach over a slice's ends; v1
   * reads such rows byte by byte), marks every tile it has ops in */
  if (!tile_flag) return;
  const bool inside = d.t_src_off >= 32ull && d.t_src_off + d.t_src_len + 32ull <= t_fa_bytes && d.q_src_off >= 32ull &&
                      d.q_src_off + d.q_src_len + 32ull <= q_fa_bytes;
  if ((d.neg & 0xEull) == 0ull && inside) return;
  const u64 a = op_off[r], b = op_off[r + 1];
  if (b <= a) return;
  for (u64 t = a / WGA_TILE; t <= (b - 1) / WGA_TILE; t++) tile_flag[t] = 1;
}

/* One thread per tile: class sums of the tile's first record before the tile = tail of the tile
 * where the record starts + totals of the tiles in between, plus everything else the expand
 * kernel wants to know up front (wga_tile_desc).  Walk-backs over more than 64 tiles (records
 * beyond 64 kop) are summed by the whole wave, one such tile at a time. */
/* pseudo != 0 (pafpseudo's rows, wga_kernels_k2s.h): S ops count as I (both skip query bases without a column), and a tile's
 * "columns" are everything it makes a row kernel walk (M = X I D S). */
/* The streaming row kernel's pre-pass (tile_flag != NULL): a tile one of its records flagged (k_rec_desc / k_pseudo_rec_desc),
 * a tile wider than that kernel takes, and every tile under `all_slow` is left to v1: WGA_S_SKIP in its descriptor, bit
 * (tile - first tile of its job) in the job's word of job_skip (all ones under all_slow) — the one word a wave of the streaming
 * kernel reads — and an entry in v1's lists: counts[0] / list_fast its row emitters, counts[1] / list_slow (beyond 2^31 columns,
 * all_slow) the op-serial walk.  The flags, the counters and the job words are cleared in front of the pre-pass. */
#define WGA_S_MAX_TILE_COLS (1ull << 24) /* wider tiles are left to v1 */
#define WGA_S_SKIP 0x100u                /* wga_tile_desc::neg: the streaming kernel leaves this tile to v1 */
__global__ __launch_bounds__(256) void k_tile_base(const u64* op_off, u64 n_ops,
                                                   const wga_tile_sum* tiles,
                                                   const wga_rec_desc* recs, wga_tile_desc* descs, int pseudo,
                                                   const u8* tile_flag, u32 job_tiles, int all_slow, u32* job_skip,
                                                   u32* counts, u32* list_fast, u32* list_slow) {
  const u32 lane = threadIdx.x & 63u;
  const u64 g = (u64)blockIdx.x * 256 + threadIdx.x;
  const u64 tile_start = g * WGA_TILE;
  const bool valid = tile_start < n_ops;
  wga_tile_sum ts;
  u64 rs = 0, re = 0, g0 = 0;
  if (valid) {
    ts = tiles[g];
    rs = op_off[ts.rec];
    re = op_off[ts.rec + 1];
  }
  u64 p_mx = 0, p_i = 0, p_d = 0;
  bool far = false;
  if (valid && rs < tile_start) {
    g0 = rs / WGA_TILE;
    if (g - g0 <= 64) {
      for (u64 k = g0; k < g; k++) {
        const u64* v = (k == g0) ? tiles[k].tail : tiles[k].tot;
        p_mx += v[CLS_MX];
        p_i += v[CLS_I] + (pseudo ? v[CLS_S] : 0ull);
        p_d += v[CLS_D];
      }
    } else {
      far = true;
    }
  }
  u64 m = __ballot(far);
  while (m) {
    const int src = (int)__builtin_ctzll(m);
    const u64 gg = __shfl(g, src), gg0 = __shfl(g0, src);
    u64 a_mx = 0, a_i = 0, a_d = 0;
    for (u64 k = gg0 + lane; k < gg; k += 64) {
      const u64* v = (k == gg0) ? tiles[k].tail : tiles[k].tot;
      a_mx += v[CLS_MX];
      a_i += v[CLS_I] + (pseudo ? v[CLS_S] : 0ull);
      a_d += v[CLS_D];
    }
    a_mx = wave_sum_u64(a_mx);
    a_i = wave_sum_u64(a_i);
    a_d = wave_sum_u64(a_d);
    if ((int)lane == src) {
      p_mx = a_mx;
      p_i = a_i;
      p_d = a_d;
    }
    m &= m - 1;
  }
  if (!valid) return;
  const wga_rec_desc rd = recs[ts.rec];
  wga_tile_desc d;
  d.tile_cols = ts.tot[CLS_MX] + ts.tot[CLS_I] + ts.tot[CLS_D] + (pseudo ? ts.tot[CLS_S] : 0ull);
  d.rec = (u32)ts.rec;
  d.neg = (u32)rd.neg;
  if (tile_flag) {
    const bool slow = all_slow || d.tile_cols > WGA_FAST_COL_LIMIT;
    if (slow || tile_flag[g] || d.tile_cols > WGA_S_MAX_TILE_COLS) {
      d.neg |= WGA_S_SKIP;
      atomicOr(&job_skip[g / job_tiles], all_slow ? 0xFFFFFFFFu : 1u << (u32)(g % job_tiles));
      if (slow)
        list_slow[atomicAdd(&counts[1], 1u)] = (u32)g;
      else
        list_fast[atomicAdd(&counts[0], 1u)] = (u32)g;
    }
  }
  d.b_mx = p_mx;
  d.b_i = p_i;
  d.b_d = p_d;
  d.rs = rs;
  d.re = re;
  d.t_row_off = rd.t_row_off;
  d.q_row_off = rd.q_row_off;
  d.t_src_off = rd.t_src_off;
  d.t_src_len = rd.t_src_len;
  d.q_src_off = rd.q_src_off;
  d.q_src_len = rd.q_src_len;
  d.I_total = rd.I_total;
  d.D_total = rd.D_total;
  d.L = rd.L;
  descs[g] = d;
}

/* the arguments of the row kernels: K2s (wga_kernels_k2s.h) and v1 (wga_k2_v1.h) */
struct ExpandArgs {
  const u32* ops;
  const u64* op_off;
  u64 n_ops;
  const wga_tile_desc* tdesc;
  const wga_rec_desc* recs;
  const u8* t_fa;
  u64 t_fa_bytes;
  const u8* q_fa;
  u64 q_fa_bytes;
  u8* out;
  wga_rec_diag* diag;
  int force_slow;
  int no_table; /* test knob: 256-column granules (the coarse-table path of very wide tiles) */
  u32 drain_min; /* RowSrc::drain_min of the rows */
  const u32* tile_count; /* k_paf2maf_expand_list: the blocks loop over tile_list[0 .. *tile_count) */
  const u32* tile_list;
  u32 n_rec;    /* records of the batch (op_off has n_rec + 1 entries) */
  u32 job_tiles;   /* streaming kernel: consecutive tiles one wave walks as one stream */
  const u32* job_skip; /* ... one word per job: bit k = tile (first tile of the job) + k is left to v1 (k_tile_base) */
};

#endif /* WGA_KERNELS_H */
