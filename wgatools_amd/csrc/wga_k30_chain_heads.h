/*
 * wga_k30_chain_heads.h — K30: the chain heads of `paf2chain` and `maf2chain` (ChainHeader's Display, chain.rs:185-203, behind the
 * TryFrom arithmetic of chain.rs:103-183) and the "\n\n" that ends a record, written around K10's data lines.
 * One header per kernel family; wga_capi.cpp includes them in dependency order (a header may use helpers of the ones in front of it).
 */
#ifndef WGA_K30_CHAIN_HEADS_H
#define WGA_K30_CHAIN_HEADS_H

#include "wga_text_out.h" /* the sinks, the staged stretch */
#include "wga_paf_head.h" /* name_span_len */

/* ============================================================================================ */
/* K30: chain heads                                                                             */
/* ============================================================================================ */
/* Record r of a batch is
 *   chain\t255\t<tname>\t<t0>\t+\t<ts>\t<te>\t<qname>\t<q0>\t<+|->\t<qs>\t<qe>\t<chain_id0 + r>      the head (K30)
 *   \n<size>\t<dt>\t<dq> ... \n<size>                                                                 nbytes[r] bytes (K10)
 *   \n\n                                                                                              (K30)
 * and the records stand back to back up to the first one K10 found an op outside M = X I D in (n_good).  The head's numbers come
 * from the caller's wga_maf2paf_head (size, start, end of both sides, before trimming) and K10's trims, all mod 2^64.
 *   plan   one thread per record: the head's byte count (the emitter into a TextCount), and n_good by atomicMin.
 *   scan   the exclusive scan of head + nbytes + 2 over the records in front of n_good (0 from there on): a record's place.
 *   place  data_off[r] = the place of K10's text of record r.
 *   fill   one wave per record.  The head of record r and the "\n\n" of record r - 1 are adjacent, so the wave's stretch is
 *          [rec_off[r] - 2, rec_off[r] + head) ([rec_off[0], ..) for the first record): lane 0 runs the emitter into the
 *          wave's stage, the wave flushes it in 16-byte stores.  A stretch longer than the stage (a name of kilobytes) is
 *          written where it belongs.  The wave of the last record also writes the two bytes that end the text.  Nothing else is
 *          touched: K10's fill owns the gaps. */
#define WGA_CHAIN_HEADS_STAGE 512u

struct ChainHeadNums {
  u64 ts, te, qs, qe;
};
/* chain.rs:103-183: the printed coordinates.  On the '-' strand the new end is computed from the ALREADY UPDATED start
 * (chain.rs:136-137,177-178): the reference's quirk, kept. */
__device__ __forceinline__ ChainHeadNums chain_head_nums(const wga_maf2paf_head& H, const wga_chain_trim_t& T) {
  ChainHeadNums c;
  c.ts = H.t[1] + T.head_del;
  c.te = H.t[2] - T.tail_del;
  if (!H.strand_neg) {
    c.qs = H.q[1] + T.head_ins;
    c.qe = H.q[2] - T.tail_ins;
  } else {
    c.qs = H.q[0] - (H.q[2] - T.head_ins);
    c.qe = H.q[0] - (c.qs + T.tail_ins);
  }
  return c;
}

/* chain.rs:185-203 (`write!`: the names as they are, no quoting).  A name span that does not lie inside the name buffer is empty. */
template <typename S>
__device__ __forceinline__ void chain_head_emit(S& s, const wga_maf2paf_head& H, const u8* __restrict__ names, u64 n_name_bytes,
                                                const wga_chain_trim_t& T, u64 chain_id) {
  const ChainHeadNums c = chain_head_nums(H, T);
  const u32 ql = name_span_len(H.qname_off, H.qname_len, n_name_bytes), tl = name_span_len(H.tname_off, H.tname_len, n_name_bytes);
  const char* lit = "chain\t255\t";
  for (u32 k = 0; k < 10u; k++) s.c((u8)lit[k]);
  s.str(names + (tl ? H.tname_off : 0u), tl);
  s.c((u8)'\t');
  s.dec(H.t[0]);
  s.c((u8)'\t');
  s.c((u8)'+');
  s.c((u8)'\t');
  s.dec(c.ts);
  s.c((u8)'\t');
  s.dec(c.te);
  s.c((u8)'\t');
  s.str(names + (ql ? H.qname_off : 0u), ql);
  s.c((u8)'\t');
  s.dec(H.q[0]);
  s.c((u8)'\t');
  s.c(H.strand_neg ? (u8)'-' : (u8)'+');
  s.c((u8)'\t');
  s.dec(c.qs);
  s.c((u8)'\t');
  s.dec(c.qe);
  s.c((u8)'\t');
  s.dec(chain_id);
}

/* plan[r] = the bytes of record r's head; *n_good (all ones before the launch) = the first record with a bad op, if there is one */
__global__ __launch_bounds__(256) void k_chain_heads_plan(const u8* __restrict__ names, u64 n_name_bytes,
                                                          const wga_maf2paf_head* __restrict__ heads, u32 n,
                                                          const wga_chain_trim_t* __restrict__ trim,
                                                          const wga_rec_diag* __restrict__ diag, u64 chain_id0,
                                                          u64* __restrict__ plan, u64* n_good) {
  const u64 r = (u64)blockIdx.x * 256u + threadIdx.x;
  if (r >= (u64)n) return;
  if (diag[r].bad_op_idx != WGA_NONE) atomicMin(n_good, r);
  TextCount t;
  chain_head_emit(t, heads[r], names, n_name_bytes, trim[r], chain_id0 + r);
  plan[r] = t.n;
}

/* scan functor: the bytes of record r — head, data lines, "\n\n" — and nothing from the first bad record on */
struct ScanChainRecs {
  const u64* plan;
  const u64* nbytes;
  const u64* n_good;
  __device__ u64 operator()(u32 r) const { return (u64)r < *n_good ? plan[r] + nbytes[r] + 2u : 0ull; }
};

/* data_off[r] = where K10 writes record r's lines: behind its head (from n_good on: the text's length, no place to write at) */
__global__ __launch_bounds__(256) void k_chain_heads_place(u32 n, const u64* __restrict__ plan, const u64* __restrict__ rec_off,
                                                           const u64* __restrict__ n_good, u64* __restrict__ data_off) {
  const u64 r = (u64)blockIdx.x * 256u + threadIdx.x;
  if (r >= (u64)n) return;
  data_off[r] = rec_off[r] + (r < *n_good ? plan[r] : 0ull);
}

/* one wave per record r < n_good.  A place that does not lie inside out[0, total) (a plan that is not this call's) is not written at. */
__global__ __launch_bounds__(256) void k_chain_heads_fill(const u8* __restrict__ names, u64 n_name_bytes,
                                                          const wga_maf2paf_head* __restrict__ heads, u32 n_good,
                                                          const wga_chain_trim_t* __restrict__ trim, u64 chain_id0,
                                                          const u64* __restrict__ plan, const u64* __restrict__ rec_off, u64 total,
                                                          u8* __restrict__ out) {
  __shared__ u32x4_a16 s_text[4][(WGA_CHAIN_HEADS_STAGE + 32u) / 16u];
  const u32 lane = threadIdx.x & 63u, wave = WGA_WAVE_ID(threadIdx.x);
  const u64 r = (u64)blockIdx.x * 4u + wave;
  if (r >= (u64)n_good) return;
  const u64 off = rec_off[r], hb = plan[r];
  const u64 lead = r ? 2u : 0u; /* the "\n\n" of the record in front */
  if (off < lead || off > total || hb > total - off) return; /* wave-uniform */
  const TextStretch st(s_text[wave], WGA_CHAIN_HEADS_STAGE, out + (off - lead), lead + hb);
  if (lane == 0u) {
    TextPut w = {st.at(0)};
    if (lead) {
      w.c((u8)'\n');
      w.c((u8)'\n');
    }
    chain_head_emit(w, heads[r], names, n_name_bytes, trim[r], chain_id0 + r);
    if (r + 1u == (u64)n_good && total - off - hb >= 2u) { /* the end of the text */
      out[total - 2u] = (u8)'\n';
      out[total - 1u] = (u8)'\n';
    }
  }
  st.flush_wave(lane);
}

#endif /* WGA_K30_CHAIN_HEADS_H */
