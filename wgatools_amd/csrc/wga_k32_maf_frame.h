/*
 * wga_k32_maf_frame.h — K32: the MAF record frames of `paf2maf` and `chain2maf` (MAFWriter::write_record, maf.rs:566-581, behind
 * the record loops of converter.rs:196-263 and :288-355): "a score=..", the heads of the two `s` lines and the blank line, written
 * around the rows of the row kernel.
 * One header per kernel family; wga_capi.cpp includes them in dependency order (a header may use helpers of the ones in front of it).
 */
#ifndef WGA_K32_MAF_FRAME_H
#define WGA_K32_MAF_FRAME_H

#include "wga_text_out.h" /* the sinks, the staged stretch */
#include "wga_paf_head.h" /* name_span_len */

/* ============================================================================================ */
/* K32: MAF record frames                                                                       */
/* ============================================================================================ */
/* Record r of a batch is
 *   a score=<score>\n
 *   s\t<tname>\t<t_start>\t<t_ali>\t<+|->\t<t_size>\t            the target head (K32)
 *   <target row: t_src_len[r] + ins_bp + inv_ins_bp bytes>        (the row kernel)
 *   \ns\t<qname>\t<q_start>\t<q_ali>\t<+|->\t<q_size>\t          the query head (K32)
 *   <query row: q_src_len[r] + del_bp + inv_del_bp bytes>         (the row kernel)
 *   \n\n                                                          (K32)
 * and the records stand back to back: ALL of them, a bad record's too (the caller cuts the text at rec_off[n_good]).
 *   plan   one thread per record: the byte counts of its two heads (the emitters into a TextCount).
 *   scan   the exclusive scan of target head + target row + query head + query row + 2: a record's place (ScanLayout's rows, so
 *          the places are wga_paf2maf_layout's for the same head lengths).
 *   place  t_row_off[r], q_row_off[r]: where the row kernel writes.
 *   fill   one wave per record, two stretches.  The "\n\n" of record r - 1, the `a` line and the target head of record r are
 *          adjacent: [rec_off[r] - 2, t_row_off[r]) ([rec_off[0], ..) for the first record).  The query head is
 *          [q_row_off[r] - its bytes, q_row_off[r]).  Lane 0 runs the first emitter and lane 1 the second, each into a stage of its
 *          own, side by side where their code is the same (the `s` line); the wave flushes both in 16-byte stores, the ragged
 *          ends in bytes.  A stretch longer than the stage (a name of kilobytes) is written where it belongs.  The wave of the
 *          last record also writes the two bytes that end the text, and lane 0 reports a record with a diagnostic (atomicMin).
 *          Nothing else is touched: the row kernel owns the gaps. */
#define WGA_MAF_FRAME_STAGE 512u

/* s\t<name>\t<start>\t<aligned size>\t<+|->\t<source size>\t  (maf.rs:570-580, `format!`: the name as it is, no quoting).  A name
 * span that does not lie inside the name buffer is empty. */
template <typename S>
__device__ __forceinline__ void maf_frame_line_emit(S& s, const u8* __restrict__ names, u64 n_name_bytes, u64 name_off, u32 name_len,
                                                    const u64* v, bool neg) {
  const u32 nl = name_span_len(name_off, name_len, n_name_bytes);
  s.c((u8)'s');
  s.c((u8)'\t');
  s.str(names + (nl ? name_off : 0u), nl);
  s.c((u8)'\t');
  s.dec(v[0]);
  s.c((u8)'\t');
  s.dec(v[1]);
  s.c((u8)'\t');
  s.c(neg ? (u8)'-' : (u8)'+');
  s.c((u8)'\t');
  s.dec(v[2]);
  s.c((u8)'\t');
}
/* side 0: "a score=<score>\n" and the target head; side 1: "\n" and the query head */
template <typename S>
__device__ __forceinline__ void maf_frame_emit(S& s, const wga_maf_frame_head& H, const u8* __restrict__ names, u64 n_name_bytes,
                                               u32 side) {
  if (!side) {
    const char* lit = "a score=";
    for (u32 k = 0; k < 8u; k++) s.c((u8)lit[k]);
    s.dec(H.score);
  }
  s.c((u8)'\n');
  maf_frame_line_emit(s, names, n_name_bytes, side ? H.qname_off : H.tname_off, side ? H.qname_len : H.tname_len,
                      (const u64*)(side ? H.q : H.t), (side ? H.q_neg : H.t_neg) != 0);
}

/* plan_t[r], plan_q[r] = the bytes of record r's two heads */
__global__ __launch_bounds__(256) void k_maf_frame_plan(const u8* __restrict__ names, u64 n_name_bytes,
                                                        const wga_maf_frame_head* __restrict__ heads, u32 n, u64* __restrict__ plan_t,
                                                        u64* __restrict__ plan_q) {
  const u64 r = (u64)blockIdx.x * 256u + threadIdx.x;
  if (r >= (u64)n) return;
  const wga_maf_frame_head H = heads[r];
  TextCount t, q;
  maf_frame_emit(t, H, names, n_name_bytes, 0u);
  maf_frame_emit(q, H, names, n_name_bytes, 1u);
  plan_t[r] = t.n;
  plan_q[r] = q.n;
}

/* scan functor: the bytes of record r — its heads, its rows (ScanLayout's, pre / post not used) and "\n\n" */
struct ScanMafRecs {
  ScanLayout rows;
  const u64* plan_t;
  const u64* plan_q;
  __device__ u64 operator()(u32 r) const { return plan_t[r] + rows.t_row(r) + plan_q[r] + rows.q_row(r) + 2u; }
};

/* the rows' places from the records' */
__global__ __launch_bounds__(256) void k_maf_frame_place(ScanMafRecs f, u32 n, const u64* __restrict__ rec_off,
                                                         u64* __restrict__ t_row_off, u64* __restrict__ q_row_off) {
  const u32 r = blockIdx.x * 256u + threadIdx.x;
  if (r >= n) return;
  const u64 t = rec_off[r] + f.plan_t[r];
  t_row_off[r] = t;
  q_row_off[r] = t + f.rows.t_row(r) + f.plan_q[r];
}

/* one wave per record.  A place that does not lie inside out[0, total) (a plan that is not this call's) is not written at.
 * *first_bad (all ones before the launch) = the first record with a diagnostic, where diag is given. */
__global__ __launch_bounds__(256) void k_maf_frame_fill(const u8* __restrict__ names, u64 n_name_bytes,
                                                        const wga_maf_frame_head* __restrict__ heads, u32 n,
                                                        const wga_rec_diag* __restrict__ diag, const u64* __restrict__ plan_t,
                                                        const u64* __restrict__ plan_q, const u64* __restrict__ rec_off,
                                                        const u64* __restrict__ q_row_off, u64 total, u8* __restrict__ out,
                                                        u64* first_bad) {
  __shared__ u32x4_a16 s_text[4][2][(WGA_MAF_FRAME_STAGE + 32u) / 16u];
  const u32 lane = threadIdx.x & 63u, wave = WGA_WAVE_ID(threadIdx.x);
  const u64 r = (u64)blockIdx.x * 4u + wave;
  if (r >= (u64)n) return;
  if (lane == 0u && diag) {
    const wga_rec_diag g = diag[r];
    if (g.bad_op_idx != WGA_NONE || g.panic_op_idx != WGA_NONE || g.bad_base_pos != WGA_NONE) atomicMin(first_bad, r);
  }
  const u64 off = rec_off[r], tb = plan_t[r], qb = plan_q[r], qend = q_row_off[r];
  const u64 lead = r ? 2u : 0u; /* the "\n\n" of the record in front */
  /* wave-uniform: both stretches inside the text, the second behind the first */
  if (off < lead || off > total || tb > total - off || qend > total || qb > qend || qend - qb < off + tb) return;
  const TextStretch st_t(s_text[wave][0], WGA_MAF_FRAME_STAGE, out + (off - lead), lead + tb);
  const TextStretch st_q(s_text[wave][1], WGA_MAF_FRAME_STAGE, out + (qend - qb), qb);
  if (lane < 2u) {
    TextPut w = {lane ? st_q.at(0) : st_t.at(0)};
    if (lane == 0u && lead) {
      w.c((u8)'\n');
      w.c((u8)'\n');
    }
    maf_frame_emit(w, heads[r], names, n_name_bytes, lane);
    if (lane == 0u && r + 1u == (u64)n && total - qend >= 2u) { /* the end of the text */
      out[total - 2u] = (u8)'\n';
      out[total - 1u] = (u8)'\n';
    }
  }
  st_t.flush_wave(lane);
  st_q.flush_wave(lane);
}

/* res[0] = *first_bad (left as it is: the host clamps it to n), res[1] = the bytes in front of that record */
__global__ __launch_bounds__(256) void k_maf_frame_result(u32 n, const u64* __restrict__ rec_off, u64* res) {
  if (blockIdx.x || threadIdx.x) return;
  const u64 g = res[0] < (u64)n ? res[0] : (u64)n;
  res[1] = rec_off[g];
}

#endif /* WGA_K32_MAF_FRAME_H */
