/* capi_paf_fix.inc — K29: `validate --fix`, the plan (which texts are taken, where the CIGARs are) and the end-fixing line writer.
 * A part of wga_capi.cpp (included there: one translation unit). */
static int paf_fix_args(const uint8_t* d_text, uint64_t n_bytes, const wga_paf_line* d_lines, uint64_t n_lines, const void* d_work) {
  if (n_lines >= 0xFFFFFFFFull || n_bytes >= 0xFFFFFFF0ull) return fail(WGA_E_INVALID_ARG, "a text within wga_paf_split's limits", nullptr);
  if (n_lines && (!d_text || !d_lines || !d_work || n_bytes == 0)) return fail(WGA_E_INVALID_ARG, "null array", nullptr);
  return WGA_OK;
}

extern "C" {

/* d_work in u64 words, the larger of the two entries' layouts.
 *   plan: header [2] | the scan of the OK flags [n + 1] | its input [n] | the newlines' positions, u32 [n]
 *   fix : header [2] | the scans of the OK flags, the rows' bytes, the two lists' bytes and the bad ends, [n + 1] each | the
 *         records, 7 words each [n] | the newlines' positions, u32 [n] */
uint64_t wga_paf_fix_work_bytes(uint64_t n_lines) { return 8ull * (12ull * n_lines + 8ull + (n_lines + 1ull) / 2ull); }

int wga_paf_fix_plan(wga_ctx* c, const uint8_t* d_text, uint64_t n_bytes, const wga_paf_line* d_lines, uint64_t n_lines, void* d_work,
                     uint64_t* n_records, uint64_t* first_untaken_line, uint64_t* d_cg_beg, uint64_t* d_cg_end) {
  int rc = ctx_bind(c);
  if (rc) return rc;
  if (!n_records || !first_untaken_line) return fail(WGA_E_INVALID_ARG, "null argument", nullptr);
  if ((rc = paf_fix_args(d_text, n_bytes, d_lines, n_lines, d_work))) return rc;
  if ((d_cg_beg == nullptr) != (d_cg_end == nullptr)) return fail(WGA_E_INVALID_ARG, "one span array without the other", nullptr);
  const u32 n = (u32)n_lines;
  K24Hdr* hdr = (K24Hdr*)d_work;
  u64* P = (u64*)d_work + 2;
  u64* val = P + n + 1u;
  u32* nl_pos = (u32*)(val + n);
  const wga_paf_line_dev* lines = (const wga_paf_line_dev*)d_lines;
  if (!d_cg_beg) {
    *n_records = 0;
    *first_untaken_line = WGA_NONE;
    if (n == 0) return WGA_OK;
    const u64* n_nl_p = nullptr;
    u64* partial = nullptr;
    if ((rc = paf_newline_list(c, d_text, n_bytes, n, nl_pos, hdr, &n_nl_p, &partial))) return rc;
    WGA_LAUNCH(k_paf_fix_plan_lines, (n + 255u) / 256u, WGA_BLOCK, c->stream, d_text, (u64)n_bytes, (u64)n, n_nl_p, (const u32*)nl_pos,
               lines, val, hdr);
    LAUNCH_CHECK();
    ScanPlain f;
    f.in = val;
    if ((rc = run_scan_ws(c, f, n, P, partial))) return rc;
    u64 tot = 0;
    K24Hdr h;
    RT_CHECK(rt_d2h(&tot, P + n, sizeof tot, c->stream));
    RT_CHECK(rt_d2h(&h, hdr, sizeof h, c->stream));
    *first_untaken_line = h.first_inexact;
    *n_records = h.first_inexact == WGA_NONE ? tot : 0u;
    return WGA_OK;
  }
  if (n == 0 || *n_records == 0) return WGA_OK;
  if (*n_records > n_lines) return fail(WGA_E_INVALID_ARG, "the counts are not the first call's", nullptr);
  WGA_LAUNCH(k_paf_fix_plan_spans, (n + 255u) / 256u, WGA_BLOCK, c->stream, (u64)n, lines, (const u64*)P, (u64*)d_cg_beg, (u64*)d_cg_end);
  LAUNCH_CHECK();
  return WGA_OK;
}

int wga_paf_fix(wga_ctx* c, const uint8_t* d_text, uint64_t n_bytes, const wga_paf_line* d_lines, uint64_t n_lines,
                const wga_cigar_counts* d_counts, uint64_t n_records, void* d_work, wga_paf_fix_sizes* sizes, uint8_t* d_rows,
                uint8_t* d_qlist, uint8_t* d_tlist) {
  int rc = ctx_bind(c);
  if (rc) return rc;
  static_assert(sizeof(wga_paf_fix_sizes) == 48, "wga_paf_fix_sizes layout");
  static_assert(sizeof(K29Rec) == 56, "K29Rec: 7 words of d_work");
  static_assert(WGA_PAF_FIX_TILE_BYTES == WGA_PAF_FIX_TILE, "the header's tile is the fill's");
  if (!sizes) return fail(WGA_E_INVALID_ARG, "sizes null", nullptr);
  if ((rc = paf_fix_args(d_text, n_bytes, d_lines, n_lines, d_work))) return rc;
  if (n_records > n_lines || (n_records && !d_counts)) return fail(WGA_E_INVALID_ARG, "d_counts[n_records] of this text's records", nullptr);
  const u32 n = (u32)n_lines;
  u64* R = (u64*)d_work + 2;
  u64* O = R + n + 1u;
  u64* QB = O + n + 1u;
  u64* TB = QB + n + 1u;
  u64* CB = TB + n + 1u;
  K29Rec* recs = (K29Rec*)(CB + n + 1u);
  u32* nl_pos = (u32*)(recs + n);
  const wga_paf_line_dev* lines = (const wga_paf_line_dev*)d_lines;
  if (!d_rows && !d_qlist && !d_tlist) {
    memset(sizes, 0, sizeof *sizes);
    if (n == 0) return WGA_OK;
    const u64* n_nl_p = nullptr;
    u64* partial = nullptr;
    if ((rc = paf_newline_list(c, d_text, n_bytes, n, nl_pos, (K24Hdr*)d_work, &n_nl_p, &partial))) return rc;
    ScanPafOk ok;
    ok.lines = lines;
    if ((rc = run_scan_ws(c, ok, n, R, partial))) return rc;
    u64 nr64 = 0;
    RT_CHECK(rt_d2h(&nr64, R + n, sizeof nr64, c->stream));
    if (nr64 != n_records) return fail(WGA_E_INVALID_ARG, "n_records is not the number of WGA_PAF_OK lines", nullptr);
    const u32 nr = (u32)nr64;
    if (nr == 0) return WGA_OK;
    WGA_LAUNCH(k_paf_fix_lines, (n + 255u) / 256u, WGA_BLOCK, c->stream, d_text, (u64)n_bytes, (u64)n, n_nl_p, (const u32*)nl_pos, lines,
               (const u64*)R, d_counts, recs);
    LAUNCH_CHECK();
    ScanFixRows fr;
    fr.recs = recs;
    if ((rc = run_scan_ws(c, fr, nr, O, partial))) return rc;
    ScanFixList<false> fq;
    fq.recs = recs, fq.lines = lines;
    if ((rc = run_scan_ws(c, fq, nr, QB, partial))) return rc;
    ScanFixList<true> ft;
    ft.recs = recs, ft.lines = lines;
    if ((rc = run_scan_ws(c, ft, nr, TB, partial))) return rc;
    ScanFixBad fb;
    fb.recs = recs;
    if ((rc = run_scan_ws(c, fb, nr, CB, partial))) return rc;
    u64 bad = 0;
    RT_CHECK(rt_d2h(&sizes->rows_bytes, O + nr, sizeof(u64), c->stream));
    RT_CHECK(rt_d2h(&sizes->qlist_bytes, QB + nr, sizeof(u64), c->stream));
    RT_CHECK(rt_d2h(&sizes->tlist_bytes, TB + nr, sizeof(u64), c->stream));
    RT_CHECK(rt_d2h(&bad, CB + nr, sizeof bad, c->stream));
    sizes->n_records = nr;
    sizes->n_q_bad = bad & 0xFFFFFFFFull;
    sizes->n_t_bad = bad >> 32;
    return WGA_OK;
  }
  if (n == 0 || sizes->n_records == 0) return WGA_OK;
  /* a row is at most its line, a newline and two numbers of 20 digits */
  if (sizes->n_records != n_records || sizes->rows_bytes < n_records || sizes->rows_bytes > n_bytes + 41ull * n_records ||
      sizes->n_q_bad > n_records || sizes->n_t_bad > n_records)
    return fail(WGA_E_INVALID_ARG, "the sizes are not the first call's", nullptr);
  const u32 nr = (u32)n_records;
  if (d_rows) {
    if (((uintptr_t)d_rows & 15u) != 0) return fail(WGA_E_INVALID_ARG, "d_rows must be 16-byte aligned", nullptr);
    const u64 tiles = (sizes->rows_bytes + WGA_PAF_FIX_TILE - 1u) / WGA_PAF_FIX_TILE;
    WGA_LAUNCH(k_paf_fix_fill, (u32)tiles, WGA_BLOCK, c->stream, d_text, (const K29Rec*)recs, (const u64*)O, nr, (u64)sizes->rows_bytes,
               d_rows);
    LAUNCH_CHECK();
  }
  u8* ql = sizes->qlist_bytes ? d_qlist : nullptr;
  u8* tl = sizes->tlist_bytes ? d_tlist : nullptr;
  if (ql || tl) {
    WGA_LAUNCH(k_paf_fix_lists, (nr + 255u) / 256u, WGA_BLOCK, c->stream, d_text, lines, (const K29Rec*)recs, nr, (const u64*)QB,
               (const u64*)TB, (u64)sizes->qlist_bytes, (u64)sizes->tlist_bytes, ql, tl);
    LAUNCH_CHECK();
  }
  return WGA_OK;
}

} /* extern "C" */
