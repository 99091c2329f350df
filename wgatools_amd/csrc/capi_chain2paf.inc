/* capi_chain2paf.inc — K27: the PAF record writer of `chain2paf` (wga_k27_chain2paf.h).
 * A part of wga_capi.cpp (included there: one translation unit; chain_items_open is there). */
/* d_work in u64 words, C = n_chains, L = n_data_lines, N = C + L items: the plan (a head's bytes) [C] | the two sums of every
 * chain [2 C] | the scan of the item sizes [N + 1] | the scans of the sizes and of the 2nd columns [2 (L + 1)] | the scans'
 * partials [N / 1024 + 4] (one scan after the other on the context's stream) */
static size_t chain2paf_work_words(uint64_t n_chains, uint64_t n_lines) {
  const uint64_t n_items = n_chains + n_lines;
  return 3 * (size_t)n_chains + (size_t)n_items + 1 + 2 * ((size_t)n_lines + 1) + (size_t)(n_items / 1024u) + 4;
}

extern "C" {

uint64_t wga_chain2paf_work_bytes(uint64_t n_chains, uint64_t n_data_lines) {
  return 8ull * (uint64_t)chain2paf_work_words(n_chains, n_data_lines);
}

int wga_chain2paf(wga_ctx* c, const uint8_t* d_text, uint64_t n_bytes, const wga_chain_head* d_heads, uint64_t n_chains,
                  const uint64_t* d_lines, const uint64_t* d_line_off, void* d_work, uint64_t* total_bytes, uint8_t* d_out) {
  int rc = ctx_bind(c);
  if (rc) return rc;
  if (!total_bytes) return fail(WGA_E_INVALID_ARG, "null argument", nullptr);
  ScanItems<Chain2PafFmt> f;
  u32 n_items;
  if ((rc = chain_items_open(c, d_text, n_bytes, d_heads, n_chains, d_lines, d_line_off, d_work, d_out, total_bytes, nullptr, &f.f,
                             &n_items)) || !n_items)
    return rc;
  const u32 nc = f.f.n_rec;
  const u64 nd = f.f.n_lines;
  u64* plan = (u64*)d_work;
  u64* sums = plan + nc;
  u64* isc = sums + 2 * (size_t)nc;
  u64* ps = isc + (size_t)n_items + 1;
  u64* pd = ps + (size_t)nd + 1;
  u64* partial = pd + (size_t)nd + 1;
  f.f.text = d_text;
  f.f.n_bytes = n_bytes;
  f.f.heads = (const wga_chain_head_dev*)d_heads;
  f.f.sums = sums;
  if (!d_out) {
    ScanChainCol col;
    col.lines = (const u64*)d_lines;
    col.col = 0u;
    if ((rc = run_scan_ws(c, col, (u32)nd, ps, partial))) return rc;
    col.col = 1u;
    if ((rc = run_scan_ws(c, col, (u32)nd, pd, partial))) return rc;
    WGA_LAUNCH(k_chain2paf_plan, (nc + 255u) / 256u, WGA_BLOCK, c->stream, d_text, (u64)n_bytes, f.f.heads, nc, (const u64*)d_line_off, nd,
               (const u64*)ps, (const u64*)pd, plan, sums);
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
