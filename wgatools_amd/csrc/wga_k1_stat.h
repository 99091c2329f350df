/*
 * wga_k1_stat.h — K1: the PAF stat walk, parse_paf_to_cigar (cigar.rs:629-707) over packed ops.
 *
 *   k_tile_rec    the record that holds the first op of every tile (one thread per tile), so that K1's waves start with
 *                 one load.
 *   k_cigar_stat  one wave per tile; 16 B/lane coalesced op loads; per-segment wave reduction; writes per-record counts
 *                 (atomics only for records that span tiles) and an 88-byte tile summary (wga_tile_sum: class sums of the
 *                 tile and of its last segment, the first op's record) that lets any later kernel place a tile inside a
 *                 long record by summing summaries instead of rescanning ops.
 */
#ifndef WGA_K1_STAT_H
#define WGA_K1_STAT_H

#include "wga_kernels.h"

#ifndef WGA_K1_BLOCKS
#define WGA_K1_BLOCKS 5 /* blocks per CU the register budget of k_cigar_stat is sized for: 94 VGPRs, no scratch.  6 (80 VGPRs + 12 B of scratch) measured 0.56 ms on one box and 0.70 ms on two others against 0.54-0.57 ms for 5 */
#endif

/* record that holds the first op of every tile: one thread per tile, plain binary search.  Done
 * ahead of the walk kernels so that their waves start with one load instead of a chain of
 * dependent probes. */
struct wga_tile_rec {
  u32 rec, neg; /* the record and its strand */
  u64 rs, re;   /* op_off[rec], op_off[rec + 1] */
};
__global__ __launch_bounds__(256) void k_tile_rec(const u64* __restrict__ op_off,
                                                  const u8* __restrict__ strand_neg, u32 n, u64 n_ops,
                                                  wga_tile_rec* __restrict__ tile_rec) {
  const u64 g = (u64)blockIdx.x * 256 + threadIdx.x;
  const u64 x = g * WGA_TILE;
  if (x >= n_ops) return;
  u32 lo = 0, hi = n; /* last r with op_off[r] <= x; op_off[0] == 0, op_off[n] == n_ops > x */
  while (hi - lo > 1u) {
    const u32 mid = lo + ((hi - lo) >> 1);
    if (op_off[mid] <= x)
      lo = mid;
    else
      hi = mid;
  }
  wga_tile_rec t;
  t.rec = lo;
  t.neg = strand_neg[lo] != 0 ? 1u : 0u;
  t.rs = op_off[lo];
  t.re = op_off[lo + 1];
  tile_rec[g] = t;
}

/* one tile of the stat walk; w = the tile's packed ops, 16 per lane: op (j*64+lane)*4+e */
__device__ __forceinline__ void cigar_stat_tile(const u64 g, const u32 (&w)[16], const u32 lane, const u64* __restrict__ op_off,
                                                const u8* __restrict__ strand_neg, u64 n_ops,
                                                const wga_tile_rec* __restrict__ tile_rec, wga_cigar_counts* counts,
                                                wga_rec_diag* diag, wga_tile_sum* tiles) {
  const u64 tile_start = g * WGA_TILE;
  const u64 tile_end = tile_start + WGA_TILE < n_ops ? tile_start + WGA_TILE : n_ops;

  /* the first segment's record, bounds and strand arrive with the ops (k_tile_rec); later
   * segments — records that start inside the tile — load theirs */
  const wga_tile_rec tr = tile_rec[g];
  u32 r = WGA_UNI32(tr.rec);
  const u32 r_first = r;
  u64 cur = tile_start;
  u64 tot[5] = {0, 0, 0, 0, 0}, tail[5] = {0, 0, 0, 0, 0};
  u64 re = WGA_UNI64(tr.re);
  /* a class sum is `len & mask`, the mask one v_bfe_i32 of a class constant by the packed op itself (bit c set: code c belongs
   * to the class; the 16 bits stand twice, so that the length's lowest bit — bit 4 of the op — picks either copy) — 17 vector
   * instructions per op (round 5: 21 with the code cut out first and the D bases summed on their own; compares and selects on
   * a class number took 45), 20 with the range test of a segment that is not the whole tile */
  constexpr u32 MX_BITS = 0x01810181u, I_BITS = 0x02020202u, X_BITS = 0x01000100u, RARE_BITS = 0xF878F878u;
  constexpr u32 IEV_BITS = 0x00020002u, DEV_BITS = 0x00040004u; /* an I (not the rest of a split one), a D */
  const u32 lane4 = lane * 4u;
  /* the wave's sums: one 32-bit reduction each when no lane's lengths add up to 2^26 (64 lanes stay below 2^32: every tile of a
   * real alignment), else two 16-bit halves each */
  auto wave_sums = [&](u32 s_mx, u32 s_i, u32 s_t, u32 s_x, u32 ev, u64& Smx, u64& Si, u64& St, u64& Sx, u32& EV) {
    if (__ballot(s_t >= (1u << 26)) == 0ull) { /* wave-uniform */
      Smx = wave_sum_u32(s_mx), Si = wave_sum_u32(s_i), St = wave_sum_u32(s_t), Sx = wave_sum_u32(s_x);
    } else {
      Smx = wave_sum_u32_wide(s_mx), Si = wave_sum_u32_wide(s_i), St = wave_sum_u32_wide(s_t), Sx = wave_sum_u32_wide(s_x);
    }
    EV = wave_sum_u32(ev);
  };
  /* The WHOLE tile first, without a range test: a tile's last segment (its only one, in four tiles of five on 5-kop records) is
   * what the segments in front leave of these sums, so only segments that end inside the tile pay the three instructions per op
   * of the test — unless the tile holds an op outside M = X I D (an error for the run: every segment is then measured on its own,
   * with its first bad op). */
  u64 Wmx, Wi, Wt, Wx;
  u32 Wev;
  bool rare_tile;
  {
    u32 s_mx = 0, s_i = 0, s_t = 0, s_x = 0, ev = 0, rare = 0;
#pragma unroll
    for (int k = 0; k < 16; k++) {
      const u32 op = w[k], len = op >> 4;
      s_mx += len & bit_mask(MX_BITS, op);
      s_i += len & bit_mask(I_BITS, op);
      s_t += len;
      s_x += len & bit_mask(X_BITS, op);
      ev += bit_test(IEV_BITS, op);
      ev += bit_test(DEV_BITS, op) << 16;
      rare |= bit_mask(RARE_BITS, op);
    }
    rare_tile = __ballot(rare != 0u) != 0ull;
    wave_sums(s_mx, s_i, s_t, s_x, ev, Wmx, Wi, Wt, Wx, Wev);
  }
  u64 Amx = 0, Ai = 0, At = 0, Ax = 0; /* the tile's segments so far */
  u32 Aev = 0;
  while (cur < tile_end) {
    while (re <= cur) { /* skip empty records */
      r++;
      re = op_off[r + 1];
    }
    const bool first = r == r_first;
    const u64 rs = first ? WGA_UNI64(tr.rs) : op_off[r];
    const bool neg = first ? (WGA_UNI32(tr.neg) != 0u) : (strand_neg[r] != 0);
    const u64 seg_end = re < tile_end ? re : tile_end;
    const u32 a = (u32)(cur - tile_start), b = (u32)(seg_end - tile_start);

    /* per-lane partials: 16 ops * (2^28-1) < 2^32, so u32 is exact.  Ops outside the segment are
     * turned into 0M (neutral) on the fly; S / other ops and the first bad op are only worked out when a wave vote
     * says the segment holds any (they end the run with an error anyway). */
    u64 S[5], Sx, St;
    u32 EV, BAD = 0xFFFFFFFFu;
    S[3] = S[4] = 0ull;
    if (!rare_tile && seg_end == tile_end) { /* wave-uniform: what the segments in front leave of the tile */
      S[0] = Wmx - Amx, S[1] = Wi - Ai, St = Wt - At, Sx = Wx - Ax;
      EV = Wev - Aev; /* both counts of the tile are at least those of its first segments: no borrow between the halves */
    } else {
      const u32 span = b - a;
      u32 s_mx = 0, s_i = 0, s_t = 0, s_s = 0, s_o = 0; /* s_t: every op's length — the D bases are what the other classes leave of it */
      u32 s_x = 0;  /* X only: match = s_mx - s_x */
      u32 ev = 0;   /* ins events | del events << 16 */
      u32 bad = 0xFFFFFFFFu;
      u32 rare = 0;
#pragma unroll
      for (int k = 0; k < 16; k++) {
        const u32 idx = (u32)(k >> 2) * 256u + (u32)(k & 3) + lane4;
        const u32 op = (idx - a < span) ? w[k] : 0u;
        const u32 len = op >> 4;
        s_mx += len & bit_mask(MX_BITS, op);
        s_i += len & bit_mask(I_BITS, op);
        s_t += len;
        s_x += len & bit_mask(X_BITS, op);
        ev += bit_test(IEV_BITS, op);
        ev += bit_test(DEV_BITS, op) << 16;
        rare |= bit_mask(RARE_BITS, op);
      }
      const bool any_rare = rare_tile && __ballot(rare != 0u) != 0ull;
      if (any_rare) {
#pragma unroll
        for (int k = 0; k < 16; k++) {
          const u32 idx = (u32)(k >> 2) * 256u + (u32)(k & 3) + lane4;
          u32 op = (idx - a < span) ? w[k] : 0u;
          WGA_PIN(op); /* opaque: no sharing of compare masks with the loop above */
          const u32 cls = op_class(op & 15u), len = op >> 4;
          s_s += cls == CLS_S ? len : 0u;
          s_o += cls == CLS_O ? len : 0u;
          bad = (cls >= CLS_S && idx < bad) ? idx : bad;
        }
      }
      wave_sums(s_mx, s_i, s_t, s_x, ev, S[0], S[1], St, Sx, EV);
      if (any_rare) {
        S[3] = wave_sum_u32_wide(s_s);
        S[4] = wave_sum_u32_wide(s_o);
        BAD = wave_min_u32(bad);
      }
      Amx += S[0], Ai += S[1], At += St, Ax += Sx, Aev += EV;
    }
    S[2] = St - S[0] - S[1] - S[3] - S[4]; /* every op is M-like, I, D, S or other */
    const u64 Smatch = S[0] - Sx;

    {
      /* the 11 counters go out from lanes 0..10, one field per lane (v_writelane from the wave-uniform sums):
       * one 88-byte store — or one atomic instruction when the record spans tiles — instead of eleven, and
       * two registers instead of twenty-two */
      const bool whole = rs >= tile_start && re <= tile_end;
      const u64 match = Smatch, mism = S[0] - Smatch;
      const u64 iev = EV & 0xFFFFu, dev = EV >> 16;
      const u64 z = 0;
      u64 v = 0;
      v = lane_put_u64<0u>(v, match, lane);
      v = lane_put_u64<1u>(v, mism, lane);
      v = lane_put_u64<2u>(v, neg ? z : iev, lane);   /* ins_ev.. or inv_ins_ev.. (cigar.rs:667-684) */
      v = lane_put_u64<3u>(v, neg ? z : S[1], lane);
      v = lane_put_u64<4u>(v, neg ? z : dev, lane);
      v = lane_put_u64<5u>(v, neg ? z : S[2], lane);
      v = lane_put_u64<6u>(v, neg ? iev : z, lane);
      v = lane_put_u64<7u>(v, neg ? S[1] : z, lane);
      v = lane_put_u64<8u>(v, neg ? dev : z, lane);
      v = lane_put_u64<9u>(v, neg ? S[2] : z, lane);
      /* inv_event = 1 per '-' record: stored with a whole record, added once by the record's first tile */
      v = lane_put_u64<10u>(v, (neg && (whole || rs >= tile_start)) ? (u64)1 : z, lane);
      u64* const f = (u64*)(counts + r);
      if (lane < 11u) {
        if (whole)
          f[lane] = v; /* the record lives in this tile only: plain stores */
        else if (v)
          atomicAdd(f + lane, v); /* record spans tiles: counts were zeroed by the launcher */
      }
      if (lane == 0 && BAD != 0xFFFFFFFFu) atomicMin((u64*)&diag[r].bad_op_idx, tile_start + BAD - rs);
    }
#pragma unroll
    for (int c = 0; c < 5; c++) {
      tot[c] += S[c];
      tail[c] = S[c];
    }
    cur = seg_end;
    r++;
    if (cur < tile_end) re = op_off[r + 1];
  }
  if (tiles) { /* wga_tile_sum = tot[5], tail[5], rec: one field per lane */
    u64 v = 0;
    v = lane_put_u64<0u>(v, tot[0], lane);
    v = lane_put_u64<1u>(v, tot[1], lane);
    v = lane_put_u64<2u>(v, tot[2], lane);
    v = lane_put_u64<3u>(v, tot[3], lane);
    v = lane_put_u64<4u>(v, tot[4], lane);
    v = lane_put_u64<5u>(v, tail[0], lane);
    v = lane_put_u64<6u>(v, tail[1], lane);
    v = lane_put_u64<7u>(v, tail[2], lane);
    v = lane_put_u64<8u>(v, tail[3], lane);
    v = lane_put_u64<9u>(v, tail[4], lane);
    v = lane_put_u64<10u>(v, (u64)r_first, lane);
    if (lane < 11u) ((u64*)(tiles + g))[lane] = v;
  }
}

/* 16 ops per lane, each of the 4 loads a fully coalesced 1 KiB.  A 16-byte group is loaded when it starts in front of the
 * stream's end (it may reach up to 12 bytes beyond it, inside the same aligned 16 bytes); what it brings from there becomes
 * 0M, as everything behind the tile's last op */
__device__ __forceinline__ void stat_load_ops(const u32* __restrict__ ops, u64 n_ops, u64 g, u32 lane, u32 (&w)[16]) {
  const u64 tile_start = g * WGA_TILE;
  const u32 nt = tile_start + WGA_TILE < n_ops ? WGA_TILE : (u32)(n_ops - tile_start);
#pragma unroll
  for (int j = 0; j < 4; j++) {
    const u32 base = ((u32)j * 64u + lane) * 4u;
    u32x4_a16 v = {0u, 0u, 0u, 0u};
    if (base < nt) v = *(const u32x4_a16*)(ops + tile_start + base);
    w[4 * j + 0] = v[0];
    w[4 * j + 1] = v[1];
    w[4 * j + 2] = v[2];
    w[4 * j + 3] = v[3];
  }
  if (nt & 3u) { /* wave-uniform: only the stream's last tile */
#pragma unroll
    for (int k = 0; k < 16; k++) w[k] = ((u32)(k >> 2) * 256u + (u32)(k & 3) + lane * 4u < nt) ? w[k] : 0u;
  }
}

/* One wave per tile.  The kernel is bound by its VECTOR instructions — a CU retires one per cycle, and 443 per tile (626 until
 * round 6: profiles/r06_pmc.txt, r05_k1_k5_counters.txt) x 487 536 tiles / 256 CUs is 0.35 of its 0.42 ms — not by its loads (a
 * plain read of the same 2 GB runs at 6.5 TB/s, scripts/micro/read_only.hip; a grid of resident waves that requested the next
 * tile's ops early: 0.586 against 0.555 ms) and not by the atomics of records that span tiles (without them: the same time). */
__global__ __launch_bounds__(256, WGA_K1_BLOCKS) void k_cigar_stat(const u32* __restrict__ ops,
                                                    const u64* __restrict__ op_off,
                                                    const u8* __restrict__ strand_neg, u32 n,
                                                    u64 n_ops, const wga_tile_rec* __restrict__ tile_rec,
                                                    wga_cigar_counts* counts,
                                                    wga_rec_diag* diag, wga_tile_sum* tiles) {
  (void)n;
  const u32 lane = threadIdx.x & 63u;
  const u64 g = (u64)blockIdx.x * 4 + WGA_WAVE_ID(threadIdx.x);
  if (g * WGA_TILE >= n_ops) return; /* wave-uniform; this kernel has no block barrier */
  u32 w[16];
  stat_load_ops(ops, n_ops, g, lane, w);
  cigar_stat_tile(g, w, lane, op_off, strand_neg, n_ops, tile_rec, counts, diag, tiles);
}

#endif /* WGA_K1_STAT_H */
