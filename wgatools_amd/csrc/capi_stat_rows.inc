/* capi_stat_rows.inc — K33: the TSV rows of `stat --each`, and the f32 formatter alone (wga_k33_stat_rows.h).
 * A part of wga_capi.cpp (included there: one translation unit; run_record_rows and run_bits_text stand there). */
extern "C" {

uint64_t wga_stat_rows_work_bytes(uint64_t n) { return 8ull * (uint64_t)record_rows_work_words(n); }

int wga_stat_rows(wga_ctx* c, uint32_t n, const uint8_t* d_names, uint64_t n_name_bytes, const wga_stat_row_head* d_heads,
                  const wga_cigar_counts* d_counts, void* d_work, uint64_t* d_row_off, uint64_t* total_bytes, uint8_t* d_out) {
  static_assert(sizeof(wga_stat_row_head) == 56 && sizeof(wga_cigar_counts) == 88, "K33's record layouts");
  int rc = ctx_bind(c);
  if (rc) return rc;
  if (!total_bytes) return fail(WGA_E_INVALID_ARG, "null argument", nullptr);
  if (!d_work) return fail(WGA_E_INVALID_ARG, "d_work null", nullptr);
  if (n > 0xFFFFFFF0u) return fail(WGA_E_INVALID_ARG, "more than 0xFFFFFFF0 rows", nullptr);
  /* d_names may be null when no name has a byte: every span is then outside the buffer */
  if (n && (!d_heads || !d_counts || !d_row_off || (n_name_bytes && !d_names))) return fail(WGA_E_INVALID_ARG, "null array", nullptr);
  StatRowsFmt f;
  f.names = d_names;
  f.n_name_bytes = d_names ? n_name_bytes : 0u;
  f.heads = d_heads;
  f.counts = d_counts;
  return run_record_rows(c, f, n, d_work, d_row_off, total_bytes, d_out);
}

int wga_f32_text(wga_ctx* c, uint64_t n, const uint32_t* d_bits, uint8_t* d_text, uint8_t* d_len) {
  return run_bits_text<u32, 16u, f32_text_emit<TextPut>>(c, n, d_bits, d_text, d_len);
}

} /* extern "C" */
