/* capi_pafpseudo.inc — K6: pafpseudo (class sums, the fill).
 * A part of wga_capi.cpp (included there: one translation unit). */
static CallKey class_tab_key(const wga_cigar_batch* b) {
  return {6, {{b->d_ops, (size_t)b->n_ops * 4}, {b->d_op_off, ((size_t)b->n + 1) * 8}}, {b->n, b->n_ops}};
}

extern "C" {

/* The class sums are the count call of pafpseudo's protocol (the host sizes the row segments from them): the tile sums and the
 * record sums stay in the context for wga_pafpseudo_fill on the same batch (keyed by its arrays and counts, dropped when one of
 * them is freed), which then is the fill kernel alone. */
int wga_cigar_class_sums(wga_ctx* c, const wga_cigar_batch* b, wga_class_sums* d_sums) {
  int rc = ctx_bind(c);
  if (rc) return rc;
  if ((rc = check_batch(b))) return rc;
  if (b->n == 0) return WGA_OK;
  if (!d_sums) return fail(WGA_E_INVALID_ARG, "d_sums null", nullptr);
  wga_ctx::ClassTab& t = c->class_tab;
  const CallKey key = class_tab_key(b);
  t.cache.take(key, false);
  u64 nt = n_tiles(b->n_ops);
  if (nt == 0) {
    RT_CHECK(rt_memset(d_sums, 0, (size_t)b->n * sizeof(wga_class_sums), c->stream));
    return WGA_OK;
  }
  const size_t tile_bytes = ((size_t)nt * sizeof(wga_tile_sum) + 63) & ~(size_t)63;
  const size_t need = tile_bytes + (size_t)b->n * sizeof(wga_class_sums);
  if ((rc = t.buf.reserve(c, need, need + need / 4))) return rc;
  t.tiles = (wga_tile_sum*)t.buf.mem;
  t.rec_sums = (wga_class_sums*)((char*)t.buf.mem + tile_bytes);
  RT_CHECK(rt_memset(t.rec_sums, 0, (size_t)b->n * sizeof(wga_class_sums), c->stream));
  WGA_LAUNCH(k_class_tiles, (u32)((nt + 3) / 4), WGA_BLOCK, c->stream, b->d_ops,
             (const u64*)b->d_op_off, b->n, (u64)b->n_ops, t.tiles, t.rec_sums);
  LAUNCH_CHECK();
  static_assert(sizeof(wga_class_sums) % 8 == 0, "wga_class_sums in 64-bit words");
  const u64 words = (u64)b->n * (sizeof(wga_class_sums) / 8);
  WGA_LAUNCH(k_copy_u64, (u32)((words + WGA_BLOCK - 1) / WGA_BLOCK), WGA_BLOCK, c->stream, words, (const u64*)t.rec_sums,
             (u64*)d_sums);
  LAUNCH_CHECK();
  t.cache.keep(key);
  return WGA_OK;
}

int wga_pafpseudo_fill(wga_ctx* c, const wga_cigar_batch* b, int base_mode, const uint8_t* d_q_fa,
                       uint64_t q_fa_bytes, const uint64_t* d_q_src_off,
                       const uint64_t* d_q_src_len, const uint64_t* d_skip, uint8_t* d_out,
                       const uint64_t* d_dst_off, wga_rec_diag* d_diag) {
  int rc = ctx_bind(c);
  if (rc) return rc;
  if ((rc = check_batch(b))) return rc;
  if (b->n == 0) return WGA_OK;
  if (!d_skip || !d_out || !d_dst_off || !d_diag) return fail(WGA_E_INVALID_ARG, "null array", nullptr);
  if (base_mode && (!d_q_fa || !d_q_src_off || !d_q_src_len))
    return fail(WGA_E_INVALID_ARG, "base mode needs the query pool", nullptr);
  RT_CHECK(rt_memset(d_diag, 0xFF, (size_t)b->n * sizeof(wga_rec_diag), c->stream));
  u64 nt = n_tiles(b->n_ops);
  if (nt == 0) return WGA_OK;
  wga_tile_sum* tiles;
  wga_class_sums* rec_sums;
  wga_ctx::ClassTab& t = c->class_tab;
  const bool kept = t.cache.take(class_tab_key(b), true); /* this fill call consumes what the class-sums call left (the sums stay where they are for this call) */
  if (nt > 0x7FFFFFFFull) return fail(WGA_E_INVALID_ARG, "batch too large for one launch", nullptr);
  /* the streaming row kernel (wga_kernels_k2s.h, MODE 2 / 3) with its pre-pass; what it leaves goes to the block kernel */
  const bool stream = c->pseudo_variant == 3;
  const size_t tile_bytes = kept ? 0 : ((size_t)nt * sizeof(wga_tile_sum) + 255) & ~(size_t)255;
  const size_t sums_bytes = kept ? 0 : ((size_t)b->n * sizeof(wga_class_sums) + 255) & ~(size_t)255;
  PrepassWs w(b->n, nt, job_tiles_for(c->expand_job_tiles, nt), true); /* behind the sums; the block kernel alone has none */
  const size_t ws_bytes = tile_bytes + sums_bytes + (stream ? w.total : 0);
  void* ws = nullptr;
  if (ws_bytes)
    if ((rc = ctx_scratch(c, ws_bytes, &ws))) return rc;
  c->pseudo_counts = nullptr;
  if (kept) {
    tiles = t.tiles; /* what wga_cigar_class_sums left for this batch */
    rec_sums = t.rec_sums;
  } else {
    tiles = (wga_tile_sum*)ws;
    rec_sums = (wga_class_sums*)((char*)ws + tile_bytes);
    RT_CHECK(rt_memset(rec_sums, 0, (size_t)b->n * sizeof(wga_class_sums), c->stream));
    WGA_LAUNCH(k_class_tiles, (u32)((nt + 3) / 4), WGA_BLOCK, c->stream, b->d_ops,
               (const u64*)b->d_op_off, b->n, (u64)b->n_ops, tiles, rec_sums);
    LAUNCH_CHECK();
  }
  PseudoArgs a;
  a.ops = b->d_ops;
  a.op_off = (const u64*)b->d_op_off;
  a.strand_neg = b->d_strand_neg;
  a.n = b->n;
  a.n_ops = b->n_ops;
  a.tiles = tiles;
  a.rec_sums = rec_sums;
  a.base_mode = base_mode;
  a.q_fa = d_q_fa;
  a.q_fa_bytes = q_fa_bytes;
  a.q_src_off = (const u64*)d_q_src_off;
  a.q_src_len = (const u64*)d_q_src_len;
  a.skip = (const u64*)d_skip;
  a.out = d_out;
  a.dst_off = (const u64*)d_dst_off;
  a.diag = d_diag;
  a.tile_count = nullptr;
  a.tile_list = nullptr;
  if (stream) {
    w.carve((char*)ws + tile_bytes + sums_bytes);
    RT_CHECK(rt_memset(w.counts, 0, w.zero_bytes, c->stream));
    WGA_LAUNCH(k_pseudo_rec_desc, (b->n + 255u) / 256u, WGA_BLOCK, c->stream, b->n, (const wga_class_sums*)rec_sums, b->d_strand_neg,
               base_mode ? (const u64*)d_q_src_off : nullptr, base_mode ? (const u64*)d_q_src_len : nullptr, (const u64*)d_skip,
               (const u64*)d_dst_off, (const u64*)b->d_op_off, (u64)q_fa_bytes, w.recs, w.tile_flag);
    LAUNCH_CHECK();
    if ((rc = launch_tile_base(c, b, w, (const wga_tile_sum*)tiles, 1, 0))) return rc;
    c->pseudo_counts = w.counts;
    ExpandArgs e;
    memset(&e, 0, sizeof(e));
    e.ops = b->d_ops;
    e.op_off = (const u64*)b->d_op_off;
    e.n_ops = b->n_ops;
    e.tdesc = w.tdesc;
    e.recs = w.recs;
    e.q_fa = base_mode ? d_q_fa : nullptr;
    e.q_fa_bytes = base_mode ? q_fa_bytes : 0;
    e.out = d_out;
    e.diag = d_diag;
    e.n_rec = b->n;
    e.job_tiles = w.job_tiles;
    e.job_skip = w.job_skip;
    if (base_mode)
      WGA_LAUNCH(k_pafpseudo_stream, (u32)((w.jobs + 1) / 2), 128u, c->stream, e);
    else
      WGA_LAUNCH(k_pafpseudo_stream_sym, (u32)((w.jobs + 1) / 2), 128u, c->stream, e);
    LAUNCH_CHECK();
    const u32 side_grid = nt < 256 ? (u32)nt : 256u;
    a.tile_count = w.counts; /* tiles of records that are not clean or lie at a pool's edge, tiles beyond 2^24 bases */
    a.tile_list = w.fast_list;
    if (base_mode)
      WGA_LAUNCH(k_pafpseudo_fill_list<true>, side_grid, WGA_BLOCK, c->stream, a);
    else
      WGA_LAUNCH(k_pafpseudo_fill_list<false>, side_grid, WGA_BLOCK, c->stream, a);
    LAUNCH_CHECK();
    a.tile_count = w.counts + 1; /* ... beyond 2^31: the block kernel decides on its op-serial walk itself */
    a.tile_list = w.wide_list;
    if (base_mode)
      WGA_LAUNCH(k_pafpseudo_fill_list<true>, side_grid, WGA_BLOCK, c->stream, a);
    else
      WGA_LAUNCH(k_pafpseudo_fill_list<false>, side_grid, WGA_BLOCK, c->stream, a);
    LAUNCH_CHECK();
    return WGA_OK;
  }
  if (base_mode)
    WGA_LAUNCH(k_pafpseudo_fill<true>, (u32)nt, WGA_BLOCK, c->stream, a);
  else
    WGA_LAUNCH(k_pafpseudo_fill<false>, (u32)nt, WGA_BLOCK, c->stream, a);
  LAUNCH_CHECK();
  return WGA_OK;
}

} /* extern "C" */
