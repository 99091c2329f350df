/* capi_paf2maf.inc — K1 / K2: stat, the scans and the layout, the row kernels of paf2maf, small helpers of that pipeline.
 * A part of wga_capi.cpp (included there: one translation unit). */
/* Tiles per job of the streaming row kernel: eight on a full-size batch; four when the whole grid is only a few rounds of the
 * device's resident waves (an eighth of configs[1] — a rank's share at 8 GPUs: 0.792 against 0.810 ms; full size: the same) */
static inline u32 job_tiles_for(int param, u64 nt) {
  if (param >= 1) return param > (int)WGA_S_MAX_JOB_TILES ? WGA_S_MAX_JOB_TILES : (u32)param;
  return nt < 200000ull ? 4u : 8u;
}

/* The workspace of the row pre-pass (k_rec_desc / k_pseudo_rec_desc, then k_tile_base), carved from the context's scratch: the
 * record descriptors, the tile descriptors, v1's two tile lists (beyond 2^31 columns; its row emitters), and behind them what ONE
 * memset clears in front of the pre-pass — the lists' two counters, and for the streaming kernel a flag byte per tile and a skip
 * word per job (without it: the counters alone, no flags, no skip words, and nothing to clear) */
struct PrepassWs {
  u64 nt, jobs;
  u32 job_tiles;
  size_t rec_bytes, desc_bytes, list_bytes, flag_bytes, skip_bytes, zero_bytes, total;
  wga_rec_desc* recs = nullptr;
  wga_tile_desc* tdesc = nullptr;
  u32 *wide_list = nullptr, *fast_list = nullptr, *counts = nullptr;
  u8* tile_flag = nullptr;
  u32* job_skip = nullptr;
  PrepassWs(u32 n, u64 nt_, u32 job_tiles_, bool stream) : nt(nt_), jobs((nt_ + job_tiles_ - 1) / job_tiles_), job_tiles(job_tiles_) {
    rec_bytes = ((size_t)n * sizeof(wga_rec_desc) + 255) & ~(size_t)255;
    desc_bytes = (size_t)nt * sizeof(wga_tile_desc);
    list_bytes = 2 * (size_t)nt * sizeof(u32);
    flag_bytes = stream ? (((size_t)nt + 255) & ~(size_t)255) : 0;
    skip_bytes = stream ? (((size_t)jobs * sizeof(u32) + 255) & ~(size_t)255) : 0;
    zero_bytes = 256 + flag_bytes + skip_bytes;
    total = rec_bytes + desc_bytes + list_bytes + zero_bytes;
  }
  void carve(void* base) {
    char* const p = (char*)base;
    recs = (wga_rec_desc*)p;
    tdesc = (wga_tile_desc*)(p + rec_bytes);
    wide_list = (u32*)(p + rec_bytes + desc_bytes);
    fast_list = wide_list + nt; /* the second half of the list area */
    counts = (u32*)(p + rec_bytes + desc_bytes + list_bytes);
    tile_flag = flag_bytes ? (u8*)counts + 256 : nullptr;
    job_skip = flag_bytes ? (u32*)(tile_flag + flag_bytes) : nullptr;
  }
};
/* k_tile_base on a carved workspace: mode 0 paf2maf's columns, 1 pafpseudo's (S ops count as I) */
static int launch_tile_base(wga_ctx* c, const wga_cigar_batch* b, const PrepassWs& w, const wga_tile_sum* tiles, int mode,
                            int force_slow) {
  WGA_LAUNCH(k_tile_base, (u32)((w.nt + 255) / 256), WGA_BLOCK, c->stream, (const u64*)b->d_op_off, (u64)b->n_ops, tiles,
             (const wga_rec_desc*)w.recs, w.tdesc, mode, (const u8*)w.tile_flag, w.job_tiles, force_slow, w.job_skip, w.counts,
             w.fast_list, w.wide_list);
  LAUNCH_CHECK();
  return WGA_OK;
}

extern "C" {

size_t wga_tile_ws_bytes(uint64_t n_ops) { return (size_t)(n_tiles(n_ops) * sizeof(wga_tile_sum)) + 16; }

int wga_cigar_stat(wga_ctx* c, const wga_cigar_batch* b, wga_cigar_counts* d_counts,
                   wga_rec_diag* d_diag, void* d_tile_ws) {
  int rc = ctx_bind(c);
  if (rc) return rc;
  if ((rc = check_batch(b))) return rc;
  if (b->n == 0) return WGA_OK;
  if (!d_counts || !d_diag) return fail(WGA_E_INVALID_ARG, "d_counts / d_diag null", nullptr);
  RT_CHECK(rt_memset(d_counts, 0, (size_t)b->n * sizeof(wga_cigar_counts), c->stream));
  RT_CHECK(rt_memset(d_diag, 0xFF, (size_t)b->n * sizeof(wga_rec_diag), c->stream));
  u64 nt = n_tiles(b->n_ops);
  if (nt == 0) return WGA_OK;
  void* ws;
  if ((rc = ctx_scratch(c, (size_t)nt * sizeof(wga_tile_rec), &ws))) return rc;
  wga_tile_rec* tile_rec = (wga_tile_rec*)ws;
  WGA_LAUNCH(k_tile_rec, (u32)((nt + 255) / 256), WGA_BLOCK, c->stream, (const u64*)b->d_op_off,
             b->d_strand_neg, b->n, (u64)b->n_ops, tile_rec);
  LAUNCH_CHECK();
  const u32 grid = (u32)((nt + 3) / 4);
  WGA_LAUNCH(k_cigar_stat, grid, WGA_BLOCK, c->stream, b->d_ops, (const u64*)b->d_op_off,
             b->d_strand_neg, b->n, (u64)b->n_ops, (const wga_tile_rec*)tile_rec, d_counts, d_diag,
             (wga_tile_sum*)d_tile_ws);
  LAUNCH_CHECK();
  return WGA_OK;
}

int wga_exclusive_scan_u64(wga_ctx* c, uint32_t n, const uint64_t* d_in, uint64_t* d_out) {
  int rc = ctx_bind(c);
  if (rc) return rc;
  if (!d_out || (n && !d_in)) return fail(WGA_E_INVALID_ARG, "null array", nullptr);
  ScanPlain f;
  f.in = (const u64*)d_in;
  return run_scan(c, f, n, (u64*)d_out);
}

int wga_paf2maf_layout(wga_ctx* c, uint32_t n, const wga_cigar_counts* d_counts,
                       const uint64_t* d_t_src_len, const uint64_t* d_q_src_len,
                       const uint32_t* d_pre_t, const uint32_t* d_pre_q, const uint32_t* d_post,
                       uint64_t* d_t_row_off, uint64_t* d_q_row_off, uint64_t* d_rec_off) {
  int rc = ctx_bind(c);
  if (rc) return rc;
  if (!d_rec_off) return fail(WGA_E_INVALID_ARG, "d_rec_off null", nullptr);
  if (n && (!d_counts || !d_t_src_len || !d_q_src_len || !d_t_row_off || !d_q_row_off))
    return fail(WGA_E_INVALID_ARG, "null array", nullptr);
  ScanLayout f;
  f.counts = d_counts;
  f.t_src_len = (const u64*)d_t_src_len;
  f.q_src_len = (const u64*)d_q_src_len;
  f.pre_t = d_pre_t;
  f.pre_q = d_pre_q;
  f.post = d_post;
  rc = run_scan(c, f, n, (u64*)d_rec_off);
  if (rc) return rc;
  if (n) {
    WGA_LAUNCH(k_layout_rows, (n + 255u) / 256u, WGA_BLOCK, c->stream, f, n, (const u64*)d_rec_off,
               (u64*)d_t_row_off, (u64*)d_q_row_off);
    LAUNCH_CHECK();
  }
  return WGA_OK;
}

int wga_paf2maf_expand(wga_ctx* c, const wga_cigar_batch* b, const wga_cigar_counts* d_counts,
                       const void* d_tile_ws, const uint8_t* d_t_fa, uint64_t t_fa_bytes,
                       const uint64_t* d_t_src_off, const uint64_t* d_t_src_len,
                       const uint8_t* d_q_fa, uint64_t q_fa_bytes, const uint64_t* d_q_src_off,
                       const uint64_t* d_q_src_len, uint8_t* d_out, const uint64_t* d_t_row_off,
                       const uint64_t* d_q_row_off, wga_rec_diag* d_diag) {
  int rc = ctx_bind(c);
  if (rc) return rc;
  if ((rc = check_batch(b))) return rc;
  if (b->n == 0 || b->n_ops == 0) return WGA_OK;
  if (!d_counts || !d_tile_ws || !d_t_src_off || !d_t_src_len || !d_q_src_off || !d_q_src_len ||
      !d_out || !d_t_row_off || !d_q_row_off || !d_diag)
    return fail(WGA_E_INVALID_ARG, "null array", nullptr);
  if ((t_fa_bytes && !d_t_fa) || (q_fa_bytes && !d_q_fa)) return fail(WGA_E_INVALID_ARG, "null sequence pool", nullptr);
  u64 nt = n_tiles(b->n_ops);
  if (nt > 0x7FFFFFFFull) return fail(WGA_E_INVALID_ARG, "batch too large for one launch", nullptr);
  /* pre-pass: per-record descriptors and per-tile base sums, in the context's scratch arena */
  const int variant = c->expand_variant >= 0 ? c->expand_variant : WGA_AUTO_LONG_VARIANT;
  c->expand_variant_used = variant;
  const bool stream = variant == 3;
  PrepassWs w(b->n, nt, job_tiles_for(c->expand_job_tiles, nt), stream);
  void* ws;
  if ((rc = ctx_scratch(c, w.total, &ws))) return rc;
  w.carve(ws);
  /* part of the pre-pass for the streaming kernel: the tiles it leaves to v1 (records that are not clean, giant tiles) —
   * k_rec_desc flags the tiles of such records, k_tile_base puts the flags into the descriptors, the jobs' skip words and
   * v1's two lists */
  if (stream) RT_CHECK(rt_memset(w.counts, 0, w.zero_bytes, c->stream));
  WGA_LAUNCH(k_rec_desc, (b->n + 255u) / 256u, WGA_BLOCK, c->stream, b->n, d_counts,
             b->d_strand_neg, (const u64*)d_t_src_off, (const u64*)d_t_src_len,
             (const u64*)d_q_src_off, (const u64*)d_q_src_len, (const u64*)d_t_row_off,
             (const u64*)d_q_row_off, w.recs, (const u64*)b->d_op_off, (u64)t_fa_bytes, (u64)q_fa_bytes, w.tile_flag);
  LAUNCH_CHECK();
  if ((rc = launch_tile_base(c, b, w, (const wga_tile_sum*)d_tile_ws, 0, c->expand_force_slow))) return rc;
  if (stream) c->stream_counts = w.counts;
  ExpandArgs a;
  a.ops = b->d_ops;
  a.op_off = (const u64*)b->d_op_off;
  a.n_ops = b->n_ops;
  a.tdesc = w.tdesc;
  a.recs = w.recs;
  a.t_fa = d_t_fa;
  a.t_fa_bytes = t_fa_bytes;
  a.q_fa = d_q_fa;
  a.q_fa_bytes = q_fa_bytes;
  a.out = d_out;
  a.diag = d_diag;
  a.force_slow = c->expand_force_slow;
  a.no_table = c->expand_no_table;
  /* when v1's waves emit their queued gap-touching chunks (RowSrc::drain_min) */
  a.drain_min = c->expand_drain_min ? c->expand_drain_min : ((u64)t_fa_bytes + (u64)q_fa_bytes > WGA_DRAIN_POOL_BYTES ? 16u : 32u);
  a.tile_count = nullptr;
  a.tile_list = nullptr;
  a.n_rec = b->n;
  a.job_tiles = w.job_tiles;
  a.job_skip = w.job_skip;
  c->expand_drain_min_used = a.drain_min;
  const uint32_t slot = c->ev_n % (uint32_t)wga_ctx::kTimingRing;
  if (c->timing) RT_CHECK(rt_event_record(c->ev[2 * slot], c->stream));
  if (stream) {
    WGA_LAUNCH(k_paf2maf_expand_s, (u32)w.jobs, 128u, c->stream, a);
    LAUNCH_CHECK();
    const u32 side_grid = nt < 256 ? (u32)nt : 256u;
    a.tile_count = w.counts; /* tiles of records that are not clean, tiles beyond 2^24 columns: v1's row emitters */
    a.tile_list = w.fast_list;
    WGA_LAUNCH(k_paf2maf_expand_list, side_grid, WGA_BLOCK, c->stream, a);
    LAUNCH_CHECK();
    a.force_slow = 1; /* beyond 2^31 columns (and everything under "expand_force_slow"): the op-serial walk */
    a.tile_count = w.counts + 1;
    a.tile_list = w.wide_list;
    WGA_LAUNCH(k_paf2maf_expand_list, side_grid, WGA_BLOCK, c->stream, a);
    LAUNCH_CHECK();
  } else {
    WGA_LAUNCH(k_paf2maf_expand, (u32)nt, WGA_BLOCK, c->stream, a);
    LAUNCH_CHECK();
  }
  if (c->timing) {
    RT_CHECK(rt_event_record(c->ev[2 * slot + 1], c->stream));
    c->ev_n++;
  }
  return WGA_OK;
}

int wga_ctx_expand_timing(wga_ctx* c, double* ms_sum, uint32_t* launches) {
  int rc = ctx_bind(c);
  if (rc) return rc;
  if (!ms_sum || !launches) return fail(WGA_E_INVALID_ARG, "null argument", nullptr);
  *ms_sum = 0.0;
  *launches = 0;
  if (!c->timing) return WGA_OK;
  const uint32_t n = c->ev_n < (uint32_t)wga_ctx::kTimingRing ? c->ev_n : (uint32_t)wga_ctx::kTimingRing;
  for (uint32_t k = 0; k < n; k++) {
    float ms = 0.0f;
    RT_CHECK(rt_event_elapsed_ms(c->ev[2 * k], c->ev[2 * k + 1], &ms));
    *ms_sum += (double)ms;
  }
  *launches = n;
  c->ev_n = 0;
  return WGA_OK;
}

int wga_scatter_bytes(wga_ctx* c, uint32_t n, const uint8_t* d_src, const uint64_t* d_src_off,
                      uint8_t* d_dst, const uint64_t* d_dst_off) {
  int rc = ctx_bind(c);
  if (rc) return rc;
  if (n == 0) return WGA_OK;
  if (!d_src || !d_src_off || !d_dst || !d_dst_off) return fail(WGA_E_INVALID_ARG, "null array", nullptr);
  WGA_LAUNCH(k_scatter_bytes, (n + 3u) / 4u, WGA_BLOCK, c->stream, n, d_src, (const u64*)d_src_off,
             d_dst, (const u64*)d_dst_off);
  LAUNCH_CHECK();
  return WGA_OK;
}

int wga_counts_total(wga_ctx* c, uint32_t n, const wga_cigar_counts* d_counts, uint64_t* d_totals) {
  int rc = ctx_bind(c);
  if (rc) return rc;
  if (!d_totals || (n && !d_counts)) return fail(WGA_E_INVALID_ARG, "null array", nullptr);
  static_assert(sizeof(wga_cigar_counts) == 88, "wga_cigar_counts is 11 u64");
  RT_CHECK(rt_memset(d_totals, 0, 88, c->stream));
  if (n == 0) return WGA_OK;
  u32 grid = (u32)(((u64)n * 11ull + 253ull * 8ull - 1ull) / (253ull * 8ull)); /* ~8 values per thread */
  if (grid > 2048u) grid = 2048u;
  WGA_LAUNCH(k_counts_total, grid, WGA_BLOCK, c->stream, n, (const u64*)d_counts, (u64*)d_totals);
  LAUNCH_CHECK();
  return WGA_OK;
}

} /* extern "C" */
