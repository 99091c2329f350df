/* capi_maf2paf.inc — K28: the PAF record writer of `maf2paf` (wga_k28_maf2paf.h).
 * A part of wga_capi.cpp (included there: one translation unit). */
/* d_work in u64 words, n blocks, R runs, N = n + R items: the plan (a head's bytes) [n] | the two sums of every block [2 n] |
 * the scan of the item sizes [N + 1] | the scan's partials [N / 1024 + 4] */
static size_t maf2paf_work_words(uint64_t n, uint64_t n_runs) {
  const uint64_t n_items = n + n_runs;
  return 3 * (size_t)n + (size_t)n_items + 1 + (size_t)(n_items / 1024u) + 4;
}

extern "C" {

uint64_t wga_maf2paf_work_bytes(uint64_t n, uint64_t n_runs) { return 8ull * (uint64_t)maf2paf_work_words(n, n_runs); }

int wga_maf2paf(wga_ctx* c, uint32_t n, const uint8_t* d_names, uint64_t n_name_bytes, const wga_maf2paf_head* d_heads,
                const wga_cigar_counts* d_counts, const uint64_t* d_runs, const uint64_t* d_run_off, const uint64_t* d_cols,
                void* d_work, uint64_t* total_bytes, uint8_t* d_out) {
  static_assert(sizeof(wga_maf2paf_head) == 80 && sizeof(wga_maf2paf_head_dev) == 80, "wga_maf2paf_head layout");
  int rc = ctx_bind(c);
  if (rc) return rc;
  if (!total_bytes) return fail(WGA_E_INVALID_ARG, "null argument", nullptr);
  if (!d_work) return fail(WGA_E_INVALID_ARG, "d_work null", nullptr);
  if (n > 0xFFFFFFF0u) return fail(WGA_E_INVALID_ARG, "more than 0xFFFFFFF0 blocks and runs", nullptr);
  /* d_names may be null when no name has a byte: every span is then outside the buffer */
  if (n && (!d_heads || !d_counts || !d_run_off || !d_cols || (n_name_bytes && !d_names)))
    return fail(WGA_E_INVALID_ARG, "null array", nullptr);
  if (!d_out) *total_bytes = 0;
  if (n == 0 || (d_out && *total_bytes == 0)) return WGA_OK;
  u64 nr = 0; /* the runs: the last offset */
  RT_CHECK(rt_d2h(&nr, d_run_off + n, sizeof nr, c->stream));
  if (nr > 0xFFFFFFF0ull || (u64)n + nr > 0xFFFFFFF0ull) return fail(WGA_E_INVALID_ARG, "more than 0xFFFFFFF0 blocks and runs", nullptr);
  if (nr && !d_runs) return fail(WGA_E_INVALID_ARG, "d_runs null", nullptr);
  const u32 n_items = (u32)((u64)n + nr);
  u64* plan = (u64*)d_work;
  u64* sums = plan + n;
  u64* isc = sums + 2 * (size_t)n;
  u64* partial = isc + (size_t)n_items + 1;
  ScanItems<Maf2PafFmt> f;
  f.f.lines = (const u64*)d_runs;
  f.f.line_off = (const u64*)d_run_off;
  f.f.plan = plan;
  f.f.n_rec = n;
  f.f.n_lines = nr;
  f.f.names = d_names;
  f.f.n_name_bytes = d_names ? n_name_bytes : 0u;
  f.f.heads = (const wga_maf2paf_head_dev*)d_heads;
  f.f.sums = sums;
  f.f.cols = (const u64*)d_cols;
  if (!d_out) {
    WGA_LAUNCH(k_maf2paf_plan, (u32)(((u64)n + 255u) / 256u), WGA_BLOCK, c->stream, f.f.names, f.f.n_name_bytes, f.f.heads, n, d_counts, plan, sums);
    LAUNCH_CHECK();
    if ((rc = run_scan_ws(c, f, n_items, isc, partial))) return rc;
    u64 tot = 0;
    RT_CHECK(rt_d2h(&tot, isc + n_items, sizeof tot, c->stream));
    *total_bytes = tot;
    return WGA_OK;
  }
  return run_text_items_fill(c, f.f, n_items, isc, (u64)*total_bytes, d_out);
}

} /* extern "C" */
