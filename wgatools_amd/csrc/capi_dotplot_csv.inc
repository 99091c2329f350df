/* capi_dotplot_csv.inc — K26: the base-level csv rows of `dotplot` (wga_k26_dotplot_csv.h).
 * A part of wga_capi.cpp (included there: one translation unit). */
/* d_work in u64 words, N rows: the row sizes, then in place their scan [N + 1] | the scan's partials [N / 1024 + 4] */
static size_t dotplot_csv_work_words(uint64_t n_rows) { return (size_t)n_rows + 1 + (size_t)(n_rows / 1024u) + 4; }

extern "C" {

uint64_t wga_dotplot_csv_work_bytes(uint64_t n_rows) { return 8ull * (uint64_t)dotplot_csv_work_words(n_rows); }

int wga_dotplot_csv(wga_ctx* c, uint32_t n, const uint64_t* d_segs, const uint64_t* d_seg_off, const uint8_t* d_tails,
                    const uint64_t* d_tail_off, void* d_work, uint64_t* total_bytes, uint8_t* d_out) {
  int rc = ctx_bind(c);
  if (rc) return rc;
  if (!total_bytes) return fail(WGA_E_INVALID_ARG, "null argument", nullptr);
  if (n && (!d_segs || !d_seg_off || !d_tails || !d_tail_off)) return fail(WGA_E_INVALID_ARG, "null array", nullptr);
  if (!d_out) *total_bytes = 0;
  if (n == 0 || (d_out && *total_bytes == 0)) return WGA_OK;
  u64 n_rows = 0; /* the last offset: read before any segment is */
  RT_CHECK(rt_d2h(&n_rows, d_seg_off + n, sizeof n_rows, c->stream));
  if (n_rows > 0xFFFFFFF0ull) return fail(WGA_E_INVALID_ARG, "more than 0xFFFFFFF0 rows", nullptr);
  if (n_rows == 0) return WGA_OK;
  if (!d_work) return fail(WGA_E_INVALID_ARG, "d_work null", nullptr);
  DotRows R;
  R.segs = (const u64*)d_segs;
  R.seg_off = (const u64*)d_seg_off;
  R.tails = (const u8*)d_tails;
  R.tail_off = (const u64*)d_tail_off;
  R.n_rec = n;
  R.n_rows = n_rows;
  u64* rsc = (u64*)d_work;
  u64* partial = rsc + (size_t)n_rows + 1;
  if (!d_out) {
    WGA_LAUNCH(k_dotplot_csv_count, (u32)((n_rows + WGA_TEXT_ITEMS - 1u) / WGA_TEXT_ITEMS), WGA_BLOCK, c->stream, R, rsc);
    LAUNCH_CHECK();
    /* the exclusive scan in place (k_scan_final reads its four values, then writes them) */
    ScanPlain f;
    f.in = rsc;
    if ((rc = run_scan_ws(c, f, (u32)n_rows, rsc, partial))) return rc;
    RT_CHECK(rt_d2h(total_bytes, rsc + n_rows, sizeof(u64), c->stream));
    return WGA_OK;
  }
  return run_text_items_fill(c, R, (u32)n_rows, rsc, (u64)*total_bytes, d_out);
}

} /* extern "C" */
