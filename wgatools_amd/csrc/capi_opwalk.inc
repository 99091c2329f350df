/* capi_opwalk.inc — K7 / K10 / K12 / K16: the op walks with their piece table of long records; K11: the element bridges.
 * A part of wga_capi.cpp (included there: one translation unit). */
static bool op_all_pieces(const wga_ctx* c, const wga_cigar_batch* b) {
  return b->n && b->n_ops > c->op_long_ops && b->n_ops / b->n > c->op_long_ops / 2;
}
/* the piece table of the op walks whose records can be long (K7, K10, K12): per record the number of pieces (0: the one-wave
 * kernel keeps it), their exclusive scan, every piece's record and `per_piece` bytes per piece, in c->op_tab.  Nothing comes
 * back to the host: the table is sized by a bound (a record of nops > long_ops ops has at most nops / piece_ops + 1 pieces,
 * and at most n_ops / long_ops records are long), t.np is that bound (0 when no record can be long) and the walks read the
 * number of pieces from piece_off[n].  With `reuse` and a table built under the same key nothing is launched (the fill
 * call of the protocol); otherwise the table is rebuilt and left invalid — the caller validates it (cache.keep) once its
 * count walk and record scan are queued. */
static int op_piece_table(wga_ctx* c, const wga_cigar_batch* b, size_t per_piece, const CallKey& key, bool reuse, bool* hit) {
  wga_ctx::OpTab& t = c->op_tab;
  *hit = t.cache.take(key, reuse); /* the fill call that takes the table consumes it (its arrays stay where they are for this call) */
  if (*hit) return WGA_OK;
  t.np = 0;
  t.all = false;
  if (b->n_ops <= c->op_long_ops) return WGA_OK;
  const u32 n = b->n;
  int rc;
  /* a batch of mostly long records: the few short ones are one piece each, so that one grid walks everything (the one-wave
   * kernel would run for the length of its longest record with the chip nearly empty) */
  t.all = op_all_pieces(c, b);
  const u64 n_long = t.all ? (u64)n : (b->n_ops / c->op_long_ops < (u64)n ? b->n_ops / c->op_long_ops : (u64)n);
  const u64 bound = b->n_ops / c->op_piece_ops + n_long + 1;
  if (bound > 0xFFFFFFF0ull) return fail(WGA_E_INVALID_ARG, "too many pieces for one call", nullptr);
  const u32 np = (u32)bound;
  const size_t head = (((size_t)n * 2 + 2 + (size_t)n / 1024 + 4) * sizeof(u64) + 63) & ~(size_t)63;
  const size_t want = head + (((size_t)np * per_piece + 63) & ~(size_t)63) + (size_t)np * sizeof(u32) + 64;
  if ((rc = t.buf.reserve(c, want, want < (1u << 20) ? (1u << 20) : want + want / 2))) return rc;
  u64* npieces = (u64*)t.buf.mem;
  u64* off = npieces + n;
  u64* partial = off + n + 1;
  WGA_LAUNCH(k_op_piece_counts, (n + 255u) / 256u, WGA_BLOCK, c->stream, n, (const u64*)b->d_op_off, (u64)c->op_long_ops,
             (u64)c->op_piece_ops, (u32)t.all, npieces);
  LAUNCH_CHECK();
  ScanPlain sp;
  sp.in = npieces;
  if ((rc = run_scan_ws(c, sp, n, off, partial))) return rc;
  t.np = np;
  t.piece_off = off;
  t.pieces = (char*)t.buf.mem + head;
  t.piece_rec = (u32*)((char*)t.pieces + (((size_t)np * per_piece + 63) & ~(size_t)63));
  WGA_LAUNCH(k_op_piece_records, (n + 255u) / 256u, WGA_BLOCK, c->stream, n, (const u64*)t.piece_off, t.piece_rec);
  LAUNCH_CHECK();
  return WGA_OK;
}
/* the key of a walk's table: the batch, the entry point's own arrays (start only) and parameters, the two piece sizes */
static CallKey op_tab_key(const wga_ctx* c, int kernel, const wga_cigar_batch* b, const void* x0, const void* x1, const void* x2,
                          uint64_t p0, uint64_t p1) {
  return {kernel,
          {{b->d_ops, (size_t)b->n_ops * 4}, {b->d_op_off, ((size_t)b->n + 1) * 8}, {x0, 0}, {x1, 0}, {x2, 0}},
          {b->n, b->n_ops, p0, p1, c->op_long_ops, c->op_piece_ops}};
}

/* K11 driver: element sizes -> exclusive scan -> per-record totals (the count call) or the fill.  The count call's scan stays for
 * the fill call of the same protocol (keyed by the entry point, its arrays and the counts, like the piece tables of K7 / K10 /
 * K12): the fill call then is the fill kernel alone — the scan it used to repeat was more than half of it.  src0, src1: the
 * arrays f reads besides the element offsets. */
template <typename F>
static int run_elems(wga_ctx* c, int kind, F f, const void* src0, const void* src1, u32 n, uint64_t n_elems,
                     const uint64_t* d_elem_off, uint64_t* d_cnt, typename F::out_t* d_out, const uint64_t* d_out_off) {
  int rc = ctx_bind(c);
  if (rc) return rc;
  if (n == 0) return WGA_OK;
  if (!d_elem_off) return fail(WGA_E_INVALID_ARG, "element offsets null", nullptr);
  if (n_elems > 0xFFFFFFF0ull) return fail(WGA_E_INVALID_ARG, "too many elements for one call", nullptr);
  if (!d_out && !d_cnt) return fail(WGA_E_INVALID_ARG, "d_cnt null", nullptr);
  if (d_out && !d_out_off) return fail(WGA_E_INVALID_ARG, "d_out_off null", nullptr);
  const u32 ne = (u32)n_elems;
  wga_ctx::ElemScan& es = c->elem_scan;
  const CallKey key = {kind, {{d_elem_off, ((size_t)n + 1) * 8}, {src0, 0}, {src1, 0}}, {n, ne}};
  if (!es.cache.take(key, d_out != nullptr)) { /* a hit is the fill call of the protocol and consumes what the count call left */
    const size_t need = ((size_t)ne + 1 + (size_t)ne / 1024 + 4) * sizeof(u64);
    if ((rc = es.buf.reserve(c, need, need + need / 4))) return rc;
    ScanElem<F> sf;
    sf.f = f;
    sf.elem_off = (const u64*)d_elem_off;
    sf.n = n;
    u64* const esc0 = (u64*)es.buf.mem;
    if ((rc = run_scan_ws(c, sf, ne, esc0, esc0 + ne + 1))) return rc;
    if (!d_out) es.cache.keep(key); /* the count call of the protocol: its scan stays */
  }
  u64* const esc = (u64*)es.buf.mem;
  if (!d_out) {
    WGA_LAUNCH(k_elem_rec_totals, (n + 255u) / 256u, WGA_BLOCK, c->stream, n, (const u64*)d_elem_off,
               (const u64*)esc, (u64*)d_cnt);
    LAUNCH_CHECK();
  } else if (ne) {
    const u32 nb = (ne + 255u) / 256u;
    void* ws;
    if ((rc = ctx_scratch(c, (size_t)nb * sizeof(wga_elem_block), &ws))) return rc;
    WGA_LAUNCH(k_elem_blocks, (nb + 255u) / 256u, WGA_BLOCK, c->stream, n, ne, (const u64*)d_elem_off, (const u64*)esc,
               (const u64*)d_out_off, (wga_elem_block*)ws);
    LAUNCH_CHECK();
    WGA_LAUNCH(k_elem_fill<F>, nb, WGA_BLOCK, c->stream, f, n, ne, (const u64*)d_elem_off, (const u64*)esc, d_out,
               (const u64*)d_out_off, (const wga_elem_block*)ws);
    LAUNCH_CHECK();
  }
  return WGA_OK;
}

static MafRunSrc maf_run_src(const uint64_t* d_runs, const uint64_t* d_run_off, const uint64_t* d_cols) {
  MafRunSrc s;
  s.runs = (const u64*)d_runs;
  s.run_off = (const u64*)d_run_off;
  s.cols = (const u64*)d_cols;
  return s;
}

extern "C" {

int wga_cigar_chain(wga_ctx* c, const wga_cigar_batch* b, wga_chain_trim_t* d_trim, uint64_t* d_nbytes,
                    wga_rec_diag* d_diag, uint8_t* d_out, const uint64_t* d_out_off) {
  int rc = ctx_bind(c);
  if (rc) return rc;
  if ((rc = check_batch(b))) return rc;
  if (b->n == 0) return WGA_OK;
  static_assert(sizeof(wga_chain_trim_t) == sizeof(wga_chain_trim), "wga_chain_trim layout");
  if (!d_out) {
    if (!d_trim || !d_nbytes || !d_diag) return fail(WGA_E_INVALID_ARG, "null array", nullptr);
    RT_CHECK(rt_memset(d_diag, 0xFF, (size_t)b->n * sizeof(wga_rec_diag), c->stream));
    if (!op_all_pieces(c, b))
      WGA_LAUNCH(k_cigar_chain<false>, (b->n + 3u) / 4u, WGA_BLOCK, c->stream, b->n, b->d_ops,
               (const u64*)b->d_op_off, (wga_chain_trim*)d_trim, (u64*)d_nbytes, d_diag, (u8*)nullptr,
               (const u64*)nullptr, (u64)c->op_long_ops);
  } else {
    if (!d_out_off) return fail(WGA_E_INVALID_ARG, "d_out_off null", nullptr);
    if (!op_all_pieces(c, b))
      WGA_LAUNCH(k_cigar_chain<true>, (b->n + 3u) / 4u, WGA_BLOCK, c->stream, b->n, b->d_ops,
               (const u64*)b->d_op_off, (wga_chain_trim*)nullptr, (u64*)nullptr, (wga_rec_diag*)nullptr,
               d_out, (const u64*)d_out_off, (u64)c->op_long_ops);
  }
  LAUNCH_CHECK();
  /* records beyond op_long_ops: pieces over the whole chip, cut where a line is certain; the count call leaves the pieces'
   * places for the fill call (op_piece_table) */
  const CallKey key = op_tab_key(c, 10, b, nullptr, nullptr, nullptr, 0, 0);
  bool hit = false;
  if ((rc = op_piece_table(c, b, sizeof(wga_chain_piece), key, d_out != nullptr, &hit))) return rc;
  const wga_ctx::OpTab& t = c->op_tab;
  if (t.np == 0) return WGA_OK;
  wga_chain_piece* pc = (wga_chain_piece*)t.pieces;
  const u32 grid = t.np < 4u * 2048u ? (t.np + 3u) / 4u : 2048u;
  if (!hit) {
    WGA_LAUNCH((k_cigar_chain_pieces<0>), grid, WGA_BLOCK, c->stream, b->n, b->d_ops, (const u64*)b->d_op_off,
               (const u64*)t.piece_off, (const u32*)t.piece_rec, pc,
               d_out ? (wga_chain_trim*)nullptr : (wga_chain_trim*)d_trim, d_out ? (wga_rec_diag*)nullptr : d_diag,
               (u8*)nullptr, (const u64*)nullptr);
    LAUNCH_CHECK();
    WGA_LAUNCH(k_cigar_chain_piece_scan, (b->n + 255u) / 256u, WGA_BLOCK, c->stream, b->n, b->d_ops, (const u64*)b->d_op_off,
               (const u64*)t.piece_off, pc, d_out ? (wga_chain_trim*)nullptr : (wga_chain_trim*)d_trim,
               d_out ? (u64*)nullptr : (u64*)d_nbytes, d_out ? (wga_rec_diag*)nullptr : d_diag);
    LAUNCH_CHECK();
    c->op_tab.cache.keep(key);
  }
  if (d_out) {
    WGA_LAUNCH((k_cigar_chain_pieces<1>), grid, WGA_BLOCK, c->stream, b->n, b->d_ops, (const u64*)b->d_op_off,
               (const u64*)t.piece_off, (const u32*)t.piece_rec, pc, (wga_chain_trim*)nullptr,
               (wga_rec_diag*)nullptr, d_out, (const u64*)d_out_off);
    LAUNCH_CHECK();
  }
  return WGA_OK;
}

int wga_cigar_dotplot(wga_ctx* c, const wga_cigar_batch* b, uint64_t cutoff, const uint64_t* d_t_start,
                      const uint64_t* d_q_start, uint64_t* d_seg_cnt, uint64_t* d_segs,
                      const uint64_t* d_seg_off) {
  int rc = ctx_bind(c);
  if (rc) return rc;
  if ((rc = check_batch(b))) return rc;
  if (b->n == 0) return WGA_OK;
  if (!d_t_start || !d_q_start) return fail(WGA_E_INVALID_ARG, "start arrays null", nullptr);
  if (!d_segs) {
    if (!d_seg_cnt) return fail(WGA_E_INVALID_ARG, "d_seg_cnt null", nullptr);
    if (!op_all_pieces(c, b))
      WGA_LAUNCH(k_dotplot_segments<false>, (b->n + 3u) / 4u, WGA_BLOCK, c->stream, b->n, b->d_ops,
               (const u64*)b->d_op_off, b->d_strand_neg, (u64)cutoff, (const u64*)d_t_start,
               (const u64*)d_q_start, (u64*)d_seg_cnt, (u64*)nullptr, (const u64*)nullptr, (u64)c->op_long_ops);
  } else {
    if (!d_seg_off) return fail(WGA_E_INVALID_ARG, "d_seg_off null", nullptr);
    if (!op_all_pieces(c, b))
      WGA_LAUNCH(k_dotplot_segments<true>, (b->n + 3u) / 4u, WGA_BLOCK, c->stream, b->n, b->d_ops,
               (const u64*)b->d_op_off, b->d_strand_neg, (u64)cutoff, (const u64*)d_t_start,
               (const u64*)d_q_start, (u64*)nullptr, (u64*)d_segs, (const u64*)d_seg_off, (u64)c->op_long_ops);
  }
  LAUNCH_CHECK();
  /* records beyond op_long_ops: pieces over the whole chip (as in wga_paf_call_events) */
  const CallKey key = op_tab_key(c, 12, b, b->d_strand_neg, d_t_start, d_q_start, cutoff, 0);
  bool hit = false;
  if ((rc = op_piece_table(c, b, sizeof(wga_dot_piece), key, d_segs != nullptr, &hit))) return rc;
  const wga_ctx::OpTab& t = c->op_tab;
  if (t.np == 0) return WGA_OK;
  wga_dot_piece* pc = (wga_dot_piece*)t.pieces;
  const u32 grid = t.np < 4u * 2048u ? (t.np + 3u) / 4u : 2048u;
  if (!hit) {
    WGA_LAUNCH((k_dotplot_pieces<0>), grid, WGA_BLOCK, c->stream, b->n, b->d_ops, (const u64*)b->d_op_off, b->d_strand_neg,
               (u64)cutoff, (const u64*)d_t_start, (const u64*)d_q_start, (const u64*)t.piece_off, (const u32*)t.piece_rec, pc, (u64*)nullptr, (const u64*)nullptr);
    LAUNCH_CHECK();
    WGA_LAUNCH(k_dotplot_piece_scan, (b->n + 255u) / 256u, WGA_BLOCK, c->stream, b->n, b->d_ops, (const u64*)b->d_op_off,
               b->d_strand_neg, (u64)cutoff, (const u64*)d_t_start, (const u64*)d_q_start, (const u64*)t.piece_off, pc,
               d_segs ? (u64*)nullptr : (u64*)d_seg_cnt);
    LAUNCH_CHECK();
    c->op_tab.cache.keep(key);
  }
  if (d_segs) {
    WGA_LAUNCH((k_dotplot_pieces<1>), grid, WGA_BLOCK, c->stream, b->n, b->d_ops, (const u64*)b->d_op_off, b->d_strand_neg,
               (u64)cutoff, (const u64*)d_t_start, (const u64*)d_q_start, (const u64*)t.piece_off, (const u32*)t.piece_rec, pc, (u64*)d_segs, (const u64*)d_seg_off);
    LAUNCH_CHECK();
  }
  return WGA_OK;
}

int wga_paf_call_events(wga_ctx* c, const wga_cigar_batch* b, uint64_t svlen, int snp,
                        uint64_t* d_ev_cnt, uint64_t* d_ev, const uint64_t* d_ev_off) {
  int rc = ctx_bind(c);
  if (rc) return rc;
  if ((rc = check_batch(b))) return rc;
  if (b->n == 0) return WGA_OK;
  if (d_ev && !d_ev_off) return fail(WGA_E_INVALID_ARG, "d_ev_off null", nullptr);
  if (!op_all_pieces(c, b))
    WGA_LAUNCH(k_paf_call_events, (b->n + 3u) / 4u, WGA_BLOCK, c->stream, b->n, b->d_ops,
             (const u64*)b->d_op_off, (u64)svlen, (u32)(snp != 0), (u64*)d_ev_cnt, (u64*)d_ev,
             (const u64*)d_ev_off, (u64)c->op_long_ops);
  LAUNCH_CHECK();
  /* records beyond op_long_ops: pieces over the whole chip; the count call walks the pieces for their sums and leaves their
   * start states for the fill call (op_piece_table), which walks them again and writes */
  const CallKey key = op_tab_key(c, 7, b, nullptr, nullptr, nullptr, svlen, snp != 0);
  bool hit = false;
  if ((rc = op_piece_table(c, b, sizeof(wga_call_piece), key, d_ev != nullptr, &hit))) return rc;
  const wga_ctx::OpTab& t = c->op_tab;
  if (t.np == 0) return WGA_OK;
  wga_call_piece* pc = (wga_call_piece*)t.pieces;
  const u32 grid = t.np < 4u * 2048u ? (t.np + 3u) / 4u : 2048u;
  if (!hit) {
    WGA_LAUNCH((k_paf_call_pieces<0>), grid, WGA_BLOCK, c->stream, b->n, b->d_ops, (const u64*)b->d_op_off, (u64)svlen,
               (u32)(snp != 0), (const u64*)t.piece_off, (const u32*)t.piece_rec, pc, (u64*)nullptr,
               (const u64*)nullptr);
    LAUNCH_CHECK();
    WGA_LAUNCH(k_paf_call_piece_scan, (b->n + 255u) / 256u, WGA_BLOCK, c->stream, b->n, (const u64*)t.piece_off, pc,
               d_ev ? (u64*)nullptr : (u64*)d_ev_cnt);
    LAUNCH_CHECK();
    c->op_tab.cache.keep(key);
  }
  if (d_ev) {
    WGA_LAUNCH((k_paf_call_pieces<1>), grid, WGA_BLOCK, c->stream, b->n, b->d_ops, (const u64*)b->d_op_off, (u64)svlen,
               (u32)(snp != 0), (const u64*)t.piece_off, (const u32*)t.piece_rec, pc, (u64*)d_ev,
               (const u64*)d_ev_off);
    LAUNCH_CHECK();
  }
  return WGA_OK;
}

int wga_paf_call_vcf(wga_ctx* c, const wga_cigar_batch* b, uint64_t svlen, const uint64_t* d_ev, const uint64_t* d_ev_off,
                     const wga_vcf_rec* d_recs, const uint8_t* d_names, const uint8_t* d_t_pool, const uint8_t* d_q_pool,
                     uint64_t* d_nbytes, wga_vcf_err* d_err, uint8_t* d_out, const uint64_t* d_out_off) {
  int rc = ctx_bind(c);
  if (rc) return rc;
  if ((rc = check_batch(b))) return rc;
  if (b->n == 0) return WGA_OK;
  static_assert(sizeof(wga_vcf_rec) == sizeof(wga_vcf_rec_dev) && sizeof(wga_vcf_rec) == 88, "wga_vcf_rec layout");
  static_assert(sizeof(wga_vcf_err) == sizeof(wga_vcf_err_dev) && sizeof(wga_vcf_err) == 16, "wga_vcf_err layout");
  if (!d_ev_off || !d_recs || !d_names || !d_t_pool || !d_q_pool) return fail(WGA_E_INVALID_ARG, "null array", nullptr);
  if (!d_out) {
    if (!d_nbytes || !d_err) return fail(WGA_E_INVALID_ARG, "null array", nullptr);
    WGA_LAUNCH(k_paf_call_vcf<false>, (b->n + 3u) / 4u, WGA_BLOCK, c->stream, b->n, b->d_ops, (const u64*)b->d_op_off,
               b->d_strand_neg, (u64)svlen, (const u64*)d_ev, (const u64*)d_ev_off, (const wga_vcf_rec_dev*)d_recs, d_names,
               d_t_pool, d_q_pool, (u64*)d_nbytes, (wga_vcf_err_dev*)d_err, (u8*)nullptr, (const u64*)nullptr);
  } else {
    if (!d_out_off) return fail(WGA_E_INVALID_ARG, "d_out_off null", nullptr);
    WGA_LAUNCH(k_paf_call_vcf<true>, (b->n + 3u) / 4u, WGA_BLOCK, c->stream, b->n, b->d_ops, (const u64*)b->d_op_off,
               b->d_strand_neg, (u64)svlen, (const u64*)d_ev, (const u64*)d_ev_off, (const wga_vcf_rec_dev*)d_recs, d_names,
               d_t_pool, d_q_pool, (u64*)nullptr, (wga_vcf_err_dev*)nullptr, d_out, (const u64*)d_out_off);
  }
  LAUNCH_CHECK();
  return WGA_OK;
}

int wga_maf_runs_ops(wga_ctx* c, uint32_t n, uint64_t n_elems, const uint64_t* d_runs, const uint64_t* d_run_off,
                     const uint64_t* d_cols, uint64_t* d_cnt, uint32_t* d_out, const uint64_t* d_out_off) {
  if (n && (!d_cols || (n_elems && !d_runs))) return fail(WGA_E_INVALID_ARG, "null array", nullptr);
  MafRunOps f;
  f.s = maf_run_src(d_runs, d_run_off, d_cols);
  return run_elems(c, 1, f, d_runs, d_cols, n, n_elems, d_run_off, d_cnt, d_out, d_out_off);
}

int wga_maf_runs_cigar_text(wga_ctx* c, uint32_t n, uint64_t n_elems, const uint64_t* d_runs,
                            const uint64_t* d_run_off, const uint64_t* d_cols, uint64_t* d_cnt, uint8_t* d_out,
                            const uint64_t* d_out_off) {
  if (n && (!d_cols || (n_elems && !d_runs))) return fail(WGA_E_INVALID_ARG, "null array", nullptr);
  MafRunText f;
  f.s = maf_run_src(d_runs, d_run_off, d_cols);
  return run_elems(c, 2, f, d_runs, d_cols, n, n_elems, d_run_off, d_cnt, d_out, d_out_off);
}

int wga_chain_lines_ops(wga_ctx* c, uint32_t n, uint64_t n_elems, const uint64_t* d_lines,
                        const uint64_t* d_line_off, uint64_t* d_cnt, uint32_t* d_out, const uint64_t* d_out_off) {
  if (n && n_elems && !d_lines) return fail(WGA_E_INVALID_ARG, "null array", nullptr);
  ChainLineOps f;
  f.s.lines = (const u64*)d_lines;
  return run_elems(c, 3, f, d_lines, nullptr, n, n_elems, d_line_off, d_cnt, d_out, d_out_off);
}

int wga_chain_lines_cigar_text(wga_ctx* c, uint32_t n, uint64_t n_elems, const uint64_t* d_lines,
                               const uint64_t* d_line_off, uint64_t* d_cnt, uint8_t* d_out,
                               const uint64_t* d_out_off) {
  if (n && n_elems && !d_lines) return fail(WGA_E_INVALID_ARG, "null array", nullptr);
  ChainLineText f;
  f.s.lines = (const u64*)d_lines;
  return run_elems(c, 4, f, d_lines, nullptr, n, n_elems, d_line_off, d_cnt, d_out, d_out_off);
}

} /* extern "C" */
