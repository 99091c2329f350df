/* capi_maf.inc — K3 / K4 / K19 / K20 / K21 / K22: the MAF walks, VCF rows of call on MAF, chunk on MAF, maf-ext's slices, the
 * block rewriter of filter and rename.
 * A part of wga_capi.cpp (included there: one translation unit). */
/* K3 / K4: the stream kernel over every block that is not long, then the long blocks piece by piece (wga_k3_maf.h).  Five
 * launches at most, all of them queued whatever the data holds: the table of long blocks is built and sized on the device (its
 * bounds — n list entries, 32 768 + n pieces — are known here), nothing is read back. */
#ifdef WGA_EMU
#define WGA_MAF_PIECE_GRID 3u /* the emulator makes 256 fibers per block, empty or not */
#else
#define WGA_MAF_PIECE_GRID 1024u /* 4 096 resident waves: a wave takes two pieces of a 10^8-column block and adds their counters up before it touches memory */
#endif
template <bool CALLER>
static int maf_walk_call(wga_ctx* c, u32 n, const u8* d_rows, const u64* d_t_off, const u64* d_q_off, const u64* d_cols,
                         const u8* d_strand_neg, wga_cigar_counts* d_counts, u64* d_run_cnt, u64* d_runs,
                         const u64* d_run_off) {
  const size_t cap = (size_t)n + WGA_MAF_PIECE_BUDGET + 1;
  const size_t o_list = 64, o_off = o_list + (((size_t)n * 4 + 63) & ~(size_t)63), o_ptot = o_off + ((((size_t)n + 1) * 4 + 63) & ~(size_t)63),
               o_ex = o_ptot + cap * sizeof(wga_maf_piece_tot), need = o_ex + (cap + 1) * sizeof(wga_maf_piece_tot);
  bool grew = false;
  int rc = c->maf_tab.reserve(c, need, need + need / 4, &grew);
  if (rc) return rc;
  if (grew || !c->maf_hdr_clean) { /* a fresh table, or a call that did not get as far as its plan */
    RT_CHECK(rt_memset(c->maf_tab.mem, 0, 64, c->stream));
    c->maf_hdr_clean = true;
  }
  char* const base = (char*)c->maf_tab.mem;
  wga_maf_long_hdr* const hdr = (wga_maf_long_hdr*)base;
  u32* const long_list = (u32*)(base + o_list);
  u32* const list_off = (u32*)(base + o_off);
  wga_maf_piece_tot* const ptot = (wga_maf_piece_tot*)(base + o_ptot);
  wga_maf_piece_tot* const ex = (wga_maf_piece_tot*)(base + o_ex);
  u32 G = c->maf_group ? c->maf_group : n / 24576u; /* eight blocks per wave where that still leaves every CU a few rounds of waves */
  G = G < 1u ? 1u : G > WGA_MAF_G ? WGA_MAF_G : G;
  const u32 grid = (u32)(((u64)n + 4ull * G - 1ull) / (4ull * G));
  /* the fill call of the two-call protocol finds the table its count call built (the long blocks, their pieces and the pieces'
   * totals): it neither lists the long blocks again nor walks them a second time for their totals */
  const size_t per_block = (size_t)n * 8;
  const CallKey key = {CALLER ? 4 : 3,
                       {{d_rows, 0}, {d_t_off, per_block}, {d_q_off, per_block}, {d_cols, per_block}, {d_strand_neg, 0}},
                       {n, c->maf_long_cols, c->maf_piece_cols}};
  const bool hit = c->maf_cache.take(key, d_runs != nullptr);
  if (!hit) c->maf_hdr_clean = false; /* until the plan has cleared the appends */
  if (d_runs)
    WGA_LAUNCH((k_maf_stream<CALLER, true>), grid, WGA_BLOCK, c->stream, n, G, d_rows, d_t_off, d_q_off, d_cols, d_strand_neg, d_counts,
               d_run_cnt, d_runs, d_run_off, (u64)c->maf_long_cols, hit ? (wga_maf_long_hdr*)nullptr : hdr, long_list);
  else
    WGA_LAUNCH((k_maf_stream<CALLER, false>), grid, WGA_BLOCK, c->stream, n, G, d_rows, d_t_off, d_q_off, d_cols, d_strand_neg, d_counts,
               d_run_cnt, d_runs, d_run_off, (u64)c->maf_long_cols, hdr, long_list);
  LAUNCH_CHECK();
  if (!hit) {
    WGA_LAUNCH(k_maf_long_plan, 1, 1024, c->stream, hdr, (const u32*)long_list, list_off, d_cols, (u64)c->maf_piece_cols);
    LAUNCH_CHECK();
    c->maf_hdr_clean = true;
    /* the fill call must not add to what the count call left in the caller's arrays */
    WGA_LAUNCH((k_maf_piece_walk<CALLER, 0>), WGA_MAF_PIECE_GRID, WGA_BLOCK, c->stream, d_rows, d_t_off, d_q_off, d_cols, d_strand_neg,
               (const wga_maf_long_hdr*)hdr, (const u32*)long_list, (const u32*)list_off, ptot, (const wga_maf_piece_tot*)nullptr,
               d_runs ? (wga_cigar_counts*)nullptr : d_counts, d_runs ? (u64*)nullptr : d_run_cnt, (u64*)nullptr, (const u64*)nullptr);
    LAUNCH_CHECK();
  }
  if (!d_runs) {
    c->maf_cache.keep(key);
    return WGA_OK;
  }
  WGA_LAUNCH(k_maf_piece_scan, 1, 1024, c->stream, (const wga_maf_long_hdr*)hdr, (const wga_maf_piece_tot*)ptot, ex);
  LAUNCH_CHECK();
  WGA_LAUNCH((k_maf_piece_walk<CALLER, 1>), WGA_MAF_PIECE_GRID, WGA_BLOCK, c->stream, d_rows, d_t_off, d_q_off, d_cols, d_strand_neg,
             (const wga_maf_long_hdr*)hdr, (const u32*)long_list, (const u32*)list_off, ptot, (const wga_maf_piece_tot*)ex,
             (wga_cigar_counts*)nullptr, (u64*)nullptr, d_runs, d_run_off);
  LAUNCH_CHECK();
  return WGA_OK;
}

extern "C" {

int wga_maf_pair_stat(wga_ctx* c, uint32_t n, const uint8_t* d_rows, const uint64_t* d_t_off,
                      const uint64_t* d_q_off, const uint64_t* d_cols,
                      const uint8_t* d_strand_neg, wga_cigar_counts* d_counts,
                      uint64_t* d_run_cnt, uint64_t* d_runs, const uint64_t* d_run_off) {
  int rc = ctx_bind(c);
  if (rc) return rc;
  if (n == 0) return WGA_OK;
  if (!d_rows || !d_t_off || !d_q_off || !d_cols || !d_strand_neg || !d_counts)
    return fail(WGA_E_INVALID_ARG, "null array", nullptr);
  if (d_runs && !d_run_off) return fail(WGA_E_INVALID_ARG, "d_run_off null", nullptr);
  return maf_walk_call<false>(c, n, d_rows, (const u64*)d_t_off, (const u64*)d_q_off, (const u64*)d_cols, d_strand_neg, d_counts,
                              (u64*)d_run_cnt, (u64*)d_runs, (const u64*)d_run_off);
}

int wga_maf_call_runs(wga_ctx* c, uint32_t n, const uint8_t* d_rows, const uint64_t* d_t_off,
                      const uint64_t* d_q_off, const uint64_t* d_cols, uint64_t* d_run_cnt,
                      uint64_t* d_runs, const uint64_t* d_run_off) {
  int rc = ctx_bind(c);
  if (rc) return rc;
  if (n == 0) return WGA_OK;
  if (!d_rows || !d_t_off || !d_q_off || !d_cols) return fail(WGA_E_INVALID_ARG, "null array", nullptr);
  if (d_runs && !d_run_off) return fail(WGA_E_INVALID_ARG, "d_run_off null", nullptr);
  return maf_walk_call<true>(c, n, d_rows, (const u64*)d_t_off, (const u64*)d_q_off, (const u64*)d_cols, (const u8*)nullptr,
                             (wga_cigar_counts*)nullptr, (u64*)d_run_cnt, (u64*)d_runs, (const u64*)d_run_off);
}

int wga_maf_call_vcf(wga_ctx* c, uint32_t n, const uint8_t* d_rows, const uint64_t* d_t_off, const uint64_t* d_q_off,
                     const uint64_t* d_cols, const uint64_t* d_runs, const uint64_t* d_run_off, const wga_maf_vcf_rec* d_recs,
                     const uint8_t* d_names, int snp, int inv, uint64_t svlen, uint64_t chunk_size, uint64_t* d_nbytes,
                     wga_vcf_err* d_err, uint8_t* d_out, const uint64_t* d_out_off) {
  int rc = ctx_bind(c);
  if (rc) return rc;
  if (n == 0) return WGA_OK;
  static_assert(sizeof(wga_maf_vcf_rec) == sizeof(wga_maf_vcf_rec_dev) && sizeof(wga_maf_vcf_rec) == 56, "wga_maf_vcf_rec layout");
  if (!d_rows || !d_t_off || !d_q_off || !d_cols || !d_runs || !d_run_off || !d_recs || !d_names)
    return fail(WGA_E_INVALID_ARG, "null array", nullptr);
  if (chunk_size == 0) return fail(WGA_E_INVALID_ARG, "chunk_size must be positive", nullptr);
  if (!d_out) {
    if (!d_nbytes || !d_err) return fail(WGA_E_INVALID_ARG, "null array", nullptr);
    WGA_LAUNCH(k_maf_call_vcf<false>, (n + 3u) / 4u, WGA_BLOCK, c->stream, n, d_rows, (const u64*)d_t_off, (const u64*)d_q_off,
               (const u64*)d_cols, (const u64*)d_runs, (const u64*)d_run_off, (const wga_maf_vcf_rec_dev*)d_recs, d_names,
               (u32)(snp != 0), (u32)(inv != 0), (u64)svlen, (u64)chunk_size, (u64*)d_nbytes, (wga_vcf_err_dev*)d_err, (u8*)nullptr,
               (const u64*)nullptr);
  } else {
    if (!d_out_off) return fail(WGA_E_INVALID_ARG, "d_out_off null", nullptr);
    WGA_LAUNCH(k_maf_call_vcf<true>, (n + 3u) / 4u, WGA_BLOCK, c->stream, n, d_rows, (const u64*)d_t_off, (const u64*)d_q_off,
               (const u64*)d_cols, (const u64*)d_runs, (const u64*)d_run_off, (const wga_maf_vcf_rec_dev*)d_recs, d_names,
               (u32)(snp != 0), (u32)(inv != 0), (u64)svlen, (u64)chunk_size, (u64*)nullptr, (wga_vcf_err_dev*)nullptr, d_out,
               (const u64*)d_out_off);
  }
  LAUNCH_CHECK();
  return WGA_OK;
}

uint64_t wga_maf_chunk_work_bytes(uint32_t n_blocks, uint64_t n_lines) {
  return 8ull * (3ull * n_lines + 2ull * (uint64_t)n_blocks + 4ull);
}

int wga_maf_chunk(wga_ctx* c, const uint8_t* d_text, const wga_maf_chunk_row* d_rows, uint32_t n_blocks,
                  const wga_maf_chunk_block* d_blocks, uint64_t n_lines, uint64_t chunk_len, uint64_t* d_carry, void* d_work,
                  uint64_t* text_bytes, uint8_t* d_out) {
  int rc = ctx_bind(c);
  if (rc) return rc;
  if (chunk_len == 0) return fail(WGA_E_INVALID_ARG, "chunk_len must be greater than 0", nullptr);
  if (n_lines >= 0xFFFFFFFFull) return fail(WGA_E_INVALID_ARG, "a window holds fewer than 2^32 lines", nullptr);
  if (!text_bytes || (n_blocks && (!d_text || !d_rows || !d_blocks || !d_carry || !d_work)))
    return fail(WGA_E_INVALID_ARG, "null array", nullptr);
  const u32 n = (u32)n_lines, nb = n_blocks;
  /* d_work: counts (then line lengths) [n] | their scan [n + 1] | the line offsets [n + 1] | the blocks' first lines [nb + 1] |
   * their first granules [nb + 1] */
  u64* A = (u64*)d_work;
  u64* pre = A + n;
  u64* loff = pre + n + 1u;
  u64* bitem = loff + n + 1u;
  u64* bgran = bitem + nb + 1u;
  if (!d_out) {
    *text_bytes = 0;
    if (n == 0) return WGA_OK;
    ScanChunkItems fi;
    fi.blocks = d_blocks;
    if ((rc = run_scan(c, fi, nb, bitem))) return rc;
    ScanChunkGran fg;
    fg.blocks = d_blocks;
    fg.rows = d_rows;
    fg.L = chunk_len;
    if ((rc = run_scan(c, fg, nb, bgran))) return rc;
    RT_CHECK(rt_memset(A, 0, (size_t)n * 8u, c->stream));
    WGA_LAUNCH(k_maf_chunk_count, WGA_K20_GRID, WGA_BLOCK, c->stream, d_text, d_rows, d_blocks, nb, (const u64*)bitem,
               (const u64*)bgran, (u64)chunk_len, A);
    LAUNCH_CHECK();
    ScanPlain f;
    f.in = A;
    if ((rc = run_scan(c, f, n, pre))) return rc;
    WGA_LAUNCH(k_maf_chunk_lines, (n + 255u) / 256u, WGA_BLOCK, c->stream, d_rows, d_blocks, nb, (const u64*)bitem,
               (const u64*)pre, (const u64*)d_carry, (u64)chunk_len, n, A);
    LAUNCH_CHECK();
    if ((rc = run_scan(c, f, n, loff))) return rc;
    u64 total = 0;
    RT_CHECK(rt_d2h(&total, loff + n, 8, c->stream));
    *text_bytes = total;
    return WGA_OK;
  }
  if (n == 0) return WGA_OK;
  const u64 tiles = (*text_bytes + WGA_MAF_TILE - 1u) / WGA_MAF_TILE;
  if (tiles >= 0x80000000ull) return fail(WGA_E_INVALID_ARG, "window text too long", nullptr);
  if (tiles) {
    WGA_LAUNCH(k_maf_chunk_fill, (u32)tiles, WGA_BLOCK, c->stream, d_text, d_rows, d_blocks, nb, (const u64*)bitem,
               (const u64*)pre, (const u64*)d_carry, (u64)chunk_len, n, (const u64*)loff, d_out);
    LAUNCH_CHECK();
  }
  WGA_LAUNCH(k_maf_chunk_carry, (nb + 255u) / 256u, WGA_BLOCK, c->stream, d_blocks, nb, (const u64*)bitem, (const u64*)pre,
             (u64*)d_carry);
  LAUNCH_CHECK();
  return WGA_OK;
}

/* d_work of K21 in u64 words: header [2] | rows' first directory entries [nr + 1] | stretch counts [E] | their scan [E + 1] |
 * hits' first lines [nh + 1] | c0 [nh] | c1 [nh] | sizes [n] | line lengths [n] | line offsets [n + 1], with E bounded by
 * n_cols / 2048 + 2 nr (a row of len columns owns ceil(len / 2048) + 1 entries) */
static inline uint64_t maf_slice_dir_bound(uint64_t n_table_rows, uint64_t n_cols) {
  return n_cols / WGA_K21_STRETCH + 2ull * n_table_rows;
}
uint64_t wga_maf_slice_work_bytes(uint32_t n_hits, uint64_t n_lines, uint64_t n_table_rows, uint64_t n_cols) {
  return 8ull * (2ull + (n_table_rows + 1ull) + 2ull * maf_slice_dir_bound(n_table_rows, n_cols) + 1ull + 3ull * (uint64_t)n_hits + 1ull +
                 3ull * n_lines + 1ull);
}

int wga_maf_slice(wga_ctx* c, const uint8_t* d_text, const wga_maf_slice_row* d_rows, uint64_t n_table_rows, uint64_t n_cols,
                  uint32_t n_hits, const wga_maf_slice_hit* d_hits, uint64_t n_lines, void* d_work, uint64_t* text_bytes,
                  uint32_t* first_short_hit, uint8_t* d_out) {
  int rc = ctx_bind(c);
  if (rc) return rc;
  static_assert(sizeof(wga_maf_slice_row) == 56 && sizeof(wga_maf_slice_hit) == 40, "K21 table layouts");
  if (n_lines >= 0xFFFFFFFFull) return fail(WGA_E_INVALID_ARG, "a window holds fewer than 2^32 lines", nullptr);
  const u64 emax = maf_slice_dir_bound(n_table_rows, n_cols);
  if (n_table_rows >= 0xFFFFFFFFull || emax >= 0xFFFFFFFFull) return fail(WGA_E_INVALID_ARG, "row table too long", nullptr);
  if (!text_bytes || !first_short_hit || (n_hits && (!d_text || !d_rows || !d_hits || !d_work)))
    return fail(WGA_E_INVALID_ARG, "null array", nullptr);
  const u32 n = (u32)n_lines, nh = n_hits, nr = (u32)n_table_rows;
  K21Hdr* hdr = (K21Hdr*)d_work;
  u64* dbase = (u64*)d_work + 2;
  u64* raw = dbase + nr + 1u;
  u64* G = raw + emax;
  u64* hline = G + emax + 1u;
  u64* C0 = hline + nh + 1u;
  u64* C1 = C0 + nh;
  u64* sz = C1 + nh;
  u64* len = sz + n;
  u64* loff = len + n;
  if (!d_out) {
    *text_bytes = 0;
    *first_short_hit = 0xFFFFFFFFu;
    if (nh == 0 || n == 0) return WGA_OK;
    RT_CHECK(rt_memset(hdr, 0xFF, sizeof(K21Hdr), c->stream));
    ScanSliceDir fd;
    fd.rows = d_rows;
    if ((rc = run_scan(c, fd, nr, dbase))) return rc;
    u64 E = 0;
    RT_CHECK(rt_d2h(&E, dbase + nr, 8, c->stream));
    if (E > emax) return fail(WGA_E_INVALID_ARG, "n_cols is smaller than the table rows' columns", nullptr);
    WGA_LAUNCH(k_maf_slice_rank, WGA_K21_GRID, WGA_BLOCK, c->stream, d_text, d_rows, nr, (const u64*)dbase, raw);
    LAUNCH_CHECK();
    ScanPlain f;
    f.in = raw;
    if ((rc = run_scan(c, f, (u32)E, G))) return rc;
    ScanSliceLines fl;
    fl.hits = d_hits;
    if ((rc = run_scan(c, fl, nh, hline))) return rc;
    WGA_LAUNCH(k_maf_slice_select, (nh + 3u) / 4u, WGA_BLOCK, c->stream, d_text, d_rows, d_hits, nh, (const u64*)dbase, (const u64*)G,
               (const u64*)hline, C0, C1, sz, hdr);
    LAUNCH_CHECK();
    WGA_LAUNCH(k_maf_slice_lines, (n + 255u) / 256u, WGA_BLOCK, c->stream, d_rows, d_hits, nh, (const u64*)hline, (const u64*)C0,
               (const u64*)C1, (const u64*)sz, (const K21Hdr*)hdr, n, len);
    LAUNCH_CHECK();
    f.in = len;
    if ((rc = run_scan(c, f, n, loff))) return rc;
    u64 total = 0;
    K21Hdr h;
    RT_CHECK(rt_d2h(&total, loff + n, 8, c->stream));
    RT_CHECK(rt_d2h(&h, hdr, sizeof h, c->stream));
    *text_bytes = total;
    *first_short_hit = h.first_short;
    return WGA_OK;
  }
  if (nh == 0 || n == 0) return WGA_OK;
  const u64 tiles = (*text_bytes + WGA_MAF_TILE - 1u) / WGA_MAF_TILE;
  if (tiles >= 0x80000000ull) return fail(WGA_E_INVALID_ARG, "window text too long", nullptr);
  if (tiles) {
    WGA_LAUNCH(k_maf_slice_fill, (u32)tiles, WGA_BLOCK, c->stream, d_text, d_rows, d_hits, nh, (const u64*)hline, (const u64*)C0,
               (const u64*)C1, (const u64*)sz, n, (const u64*)loff, d_out);
    LAUNCH_CHECK();
  }
  return WGA_OK;
}

/* d_work of K22 in u64 words: header [2] | kept blocks' places [nb + 1] | their first lines [nb + 1] | line lengths [n] | line
 * offsets [n + 1] | keep flags, u32 [nb] | the list of kept blocks, u32 [nb] */
uint64_t wga_maf_rewrite_work_bytes(uint32_t n_blocks, uint64_t n_lines) {
  return 8ull * (2ull + 2ull * ((uint64_t)n_blocks + 1ull) + 2ull * n_lines + 1ull + (uint64_t)n_blocks + 1ull);
}

int wga_maf_rewrite(wga_ctx* c, const uint8_t* d_text, const wga_maf_slice_row* d_rows, uint32_t n_blocks,
                    const wga_maf_rewrite_block* d_blocks, uint64_t n_lines, const wga_maf_rewrite_params* params, void* d_work,
                    uint64_t* text_bytes, uint32_t* n_kept, uint32_t* first_bad_block, uint8_t* d_out) {
  int rc = ctx_bind(c);
  if (rc) return rc;
  static_assert(sizeof(wga_maf_rewrite_block) == 16 && sizeof(wga_maf_rewrite_params) == 40, "K22 table layouts");
  if (n_lines >= 0xFFFFFFFFull) return fail(WGA_E_INVALID_ARG, "a window holds fewer than 2^32 lines", nullptr);
  if (!params || !text_bytes || !n_kept || !first_bad_block || (n_blocks && (!d_text || !d_rows || !d_blocks || !d_work)))
    return fail(WGA_E_INVALID_ARG, "null array", nullptr);
  if (params->n_prefix && (!params->d_prefix_text || !params->d_prefix_off))
    return fail(WGA_E_INVALID_ARG, "prefixes without their text", nullptr);
  const u32 n = (u32)n_lines, nb = n_blocks;
  const wga_maf_rewrite_params P = *params;
  K22Hdr* hdr = (K22Hdr*)d_work;
  u64* kidx = (u64*)d_work + 2;
  u64* kline = kidx + nb + 1u;
  u64* len = kline + nb + 1u;
  u64* loff = len + n;
  u32* keep = (u32*)(loff + n + 1u);
  u32* klist = keep + nb;
  if (!d_out) {
    *text_bytes = 0;
    *n_kept = 0;
    *first_bad_block = 0xFFFFFFFFu;
    if (nb == 0) return WGA_OK;
    RT_CHECK(rt_memset(hdr, 0xFF, sizeof(K22Hdr), c->stream));
    WGA_LAUNCH(k_maf_rewrite_select, (nb + 255u) / 256u, WGA_BLOCK, c->stream, d_rows, d_blocks, nb, P, keep, hdr);
    LAUNCH_CHECK();
    ScanRewriteKept fk;
    fk.keep = keep;
    fk.hdr = hdr;
    if ((rc = run_scan(c, fk, nb, kidx))) return rc;
    WGA_LAUNCH(k_maf_rewrite_compact, (nb + 255u) / 256u, WGA_BLOCK, c->stream, (const u64*)kidx, nb, klist);
    LAUNCH_CHECK();
    ScanRewriteRows fr;
    fr.blocks = d_blocks;
    fr.klist = klist;
    fr.n_kept = kidx + nb;
    if ((rc = run_scan(c, fr, nb, kline))) return rc;
    if (n) {
      WGA_LAUNCH(k_maf_rewrite_lines, (n + 255u) / 256u, WGA_BLOCK, c->stream, d_rows, d_blocks, nb, (const u32*)klist,
                 (const u64*)kidx, (const u64*)kline, P, n, len);
      LAUNCH_CHECK();
    }
    ScanPlain f;
    f.in = len;
    if ((rc = run_scan(c, f, n, loff))) return rc;
    u64 total = 0, nk = 0;
    K22Hdr h;
    RT_CHECK(rt_d2h(&total, loff + n, 8, c->stream));
    RT_CHECK(rt_d2h(&nk, kidx + nb, 8, c->stream));
    RT_CHECK(rt_d2h(&h, hdr, sizeof h, c->stream));
    *text_bytes = total;
    *n_kept = (u32)nk;
    *first_bad_block = h.first_bad;
    return WGA_OK;
  }
  if (nb == 0 || *n_kept == 0 || *text_bytes == 0) return WGA_OK;
  if (*n_kept > nb) return fail(WGA_E_INVALID_ARG, "n_kept is not the count call's", nullptr);
  const u64 tiles = (*text_bytes + WGA_MAF_TILE - 1u) / WGA_MAF_TILE;
  if (tiles >= 0x80000000ull) return fail(WGA_E_INVALID_ARG, "window text too long", nullptr);
  WGA_LAUNCH(k_maf_rewrite_fill, (u32)tiles, WGA_BLOCK, c->stream, d_text, d_rows, d_blocks, nb, (const u32*)klist, *n_kept,
             (const u64*)kline, P, (const u64*)loff, (u64)*text_bytes, d_out);
  LAUNCH_CHECK();
  return WGA_OK;
}

} /* extern "C" */
