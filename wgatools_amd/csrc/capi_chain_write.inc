/* capi_chain_write.inc — K25: the chain record writer of `filter -f chain` (wga_k25_chain_write.h).
 * A part of wga_capi.cpp (included there: one translation unit; chain_items_open is there). */
/* d_work in u64 words, N = n_chains + n_data_lines items: the plan (a head's bytes, 0 = dropped) [n_chains] | the scan of the
 * item sizes [N + 1] | the kept chains [1] (behind the scan's total: both come back in one copy) | the scan's partials
 * [N / 1024 + 4] */
static size_t chain_filter_work_words(uint64_t n_chains, uint64_t n_items) {
  return (size_t)n_chains + (size_t)n_items + 2 + (size_t)(n_items / 1024u) + 4;
}

extern "C" {

uint64_t wga_chain_filter_work_bytes(uint64_t n_chains, uint64_t n_data_lines) {
  return 8ull * (uint64_t)chain_filter_work_words(n_chains, n_chains + n_data_lines);
}

int wga_chain_filter(wga_ctx* c, const uint8_t* d_text, uint64_t n_bytes, const wga_chain_head* d_heads, uint64_t n_chains,
                     const uint64_t* d_lines, const uint64_t* d_line_off, const wga_chain_filter_params* params, void* d_work,
                     uint64_t* total_bytes, uint64_t* n_kept, uint8_t* d_out) {
  int rc = ctx_bind(c);
  if (rc) return rc;
  static_assert(sizeof(wga_chain_filter_params) == 16 && sizeof(wga_chain_filter_params) == sizeof(wga_chain_filter_params_dev),
                "K25 params layout");
  if (!params || !total_bytes || !n_kept) return fail(WGA_E_INVALID_ARG, "null argument", nullptr);
  ScanItems<ChainWriteFmt> f;
  u32 n_items;
  if ((rc = chain_items_open(c, d_text, n_bytes, d_heads, n_chains, d_lines, d_line_off, d_work, d_out, total_bytes, n_kept, &f.f,
                             &n_items)) || !n_items)
    return rc;
  f.f.text = d_text;
  f.f.heads = (const wga_chain_head_dev*)d_heads;
  const u32 nc = f.f.n_rec;
  u64* plan = (u64*)d_work;
  u64* isc = plan + nc;
  u64* kept = isc + (size_t)n_items + 1;
  u64* partial = kept + 1;
  if (!d_out) {
    wga_chain_filter_params_dev P;
    P.min_block_size = params->min_block_size;
    P.min_query_size = params->min_query_size;
    RT_CHECK(rt_memset(kept, 0, sizeof(u64), c->stream));
    WGA_LAUNCH(k_chain_write_plan, (nc + 255u) / 256u, WGA_BLOCK, c->stream, d_text, f.f.heads, nc, P, plan, kept);
    LAUNCH_CHECK();
    if ((rc = run_scan_ws(c, f, n_items, isc, partial))) return rc;
    u64 tot[2] = {0, 0};
    RT_CHECK(rt_d2h(tot, isc + n_items, sizeof tot, c->stream));
    *total_bytes = tot[0];
    *n_kept = tot[1];
    return WGA_OK;
  }
  if (*n_kept == 0 || *n_kept > n_chains) return fail(WGA_E_INVALID_ARG, "the counts are not the first call's", nullptr);
  return run_text_items_fill(c, f.f, n_items, isc, (u64)*total_bytes, d_out);
}

} /* extern "C" */
