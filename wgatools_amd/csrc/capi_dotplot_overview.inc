/* capi_dotplot_overview.inc — K34: the csv rows of `dotplot -m overview`, and the f64 formatter alone
 * (wga_k34_dotplot_overview.h).  A part of wga_capi.cpp (included there: one translation unit). */
/* d_work in u64 words, n rows: the plan (a row's bytes) [n] | the scan's partials [n / 1024 + 4] */
static size_t dotplot_ov_work_words(uint64_t n) { return (size_t)n + (size_t)(n / 1024u) + 4; }

extern "C" {

uint64_t wga_dotplot_overview_work_bytes(uint64_t n) { return 8ull * (uint64_t)dotplot_ov_work_words(n); }

int wga_dotplot_overview(wga_ctx* c, uint32_t n, const uint8_t* d_names, uint64_t n_name_bytes, const wga_dotplot_ov_head* d_heads,
                         const wga_cigar_counts* d_counts, int no_identity, void* d_work, uint64_t* d_row_off, uint64_t* total_bytes,
                         uint8_t* d_out) {
  static_assert(sizeof(wga_dotplot_ov_head) == 64 && sizeof(wga_cigar_counts) == 88, "K34's record layouts");
  int rc = ctx_bind(c);
  if (rc) return rc;
  if (!total_bytes) return fail(WGA_E_INVALID_ARG, "null argument", nullptr);
  if (!d_work) return fail(WGA_E_INVALID_ARG, "d_work null", nullptr);
  if (n > 0xFFFFFFF0u) return fail(WGA_E_INVALID_ARG, "more than 0xFFFFFFF0 rows", nullptr);
  /* d_names may be null when no name has a byte: every span is then outside the buffer; d_counts under no_identity */
  if (n && (!d_heads || (!no_identity && !d_counts) || !d_row_off || (n_name_bytes && !d_names)))
    return fail(WGA_E_INVALID_ARG, "null array", nullptr);
  if (!d_out) *total_bytes = 0;
  if (n == 0 || (d_out && *total_bytes == 0)) return WGA_OK;
  u64* plan = (u64*)d_work;
  u64* partial = plan + n;
  ScanItems<DotplotOvFmt> f;
  f.f.names = d_names;
  f.f.n_name_bytes = d_names ? n_name_bytes : 0u;
  f.f.heads = d_heads;
  f.f.counts = no_identity ? nullptr : d_counts; /* nothing is read from d_counts then */
  f.f.plan = plan;
  f.f.n_rec = n;
  if (!d_out) {
    WGA_LAUNCH(k_dotplot_ov_plan, (u32)(((u64)n + 255u) / 256u), WGA_BLOCK, c->stream, f.f.names, f.f.n_name_bytes, f.f.heads, n,
               f.f.counts, plan);
    LAUNCH_CHECK();
    if ((rc = run_scan_ws(c, f, n, (u64*)d_row_off, partial))) return rc;
    u64 tot = 0;
    RT_CHECK(rt_d2h(&tot, d_row_off + n, sizeof tot, c->stream));
    *total_bytes = tot;
    return WGA_OK;
  }
  return run_text_items_fill(c, f.f, n, (const u64*)d_row_off, (u64)*total_bytes, d_out);
}

int wga_f64_text(wga_ctx* c, uint64_t n, const uint64_t* d_bits, uint8_t* d_text, uint8_t* d_len) {
  int rc = ctx_bind(c);
  if (rc) return rc;
  if (n == 0) return WGA_OK;
  if (!d_bits || !d_text || !d_len) return fail(WGA_E_INVALID_ARG, "null array", nullptr);
  if (n > 0xFFFFFFF0ull) return fail(WGA_E_INVALID_ARG, "too many values", nullptr);
  WGA_LAUNCH(k_f64_text, (u32)((n + 255u) / 256u), WGA_BLOCK, c->stream, (u64)n, (const u64*)d_bits, d_text, d_len);
  LAUNCH_CHECK();
  return WGA_OK;
}

} /* extern "C" */
