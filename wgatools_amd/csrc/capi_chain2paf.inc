/* capi_chain2paf.inc — K27: the PAF record writer of `chain2paf` (wga_k27_chain2paf.h).
 * A part of wga_capi.cpp (included there: one translation unit). */
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
  static_assert(sizeof(wga_chain_head) == sizeof(wga_chain_head_dev), "wga_chain_head layout");
  if (!total_bytes) return fail(WGA_E_INVALID_ARG, "null argument", nullptr);
  if (!d_work) return fail(WGA_E_INVALID_ARG, "d_work null", nullptr);
  if (n_chains > 0xFFFFFFF0ull || n_bytes >= 0xFFFFFFF0ull) return fail(WGA_E_INVALID_ARG, "a text within wga_chain_split's limits", nullptr);
  if (n_chains && (!d_text || !d_heads || !d_line_off)) return fail(WGA_E_INVALID_ARG, "null array", nullptr);
  if (!d_out) *total_bytes = 0;
  if (n_chains == 0 || (d_out && *total_bytes == 0)) return WGA_OK;
  u64 nd = 0; /* the data lines: the last offset */
  RT_CHECK(rt_d2h(&nd, d_line_off + n_chains, sizeof nd, c->stream));
  if (nd > 0xFFFFFFF0ull || n_chains + nd > 0xFFFFFFF0ull) return fail(WGA_E_INVALID_ARG, "more than 0xFFFFFFF0 chains and data lines", nullptr);
  if (nd && !d_lines) return fail(WGA_E_INVALID_ARG, "d_lines null", nullptr);
  const u32 nc = (u32)n_chains, n_items = (u32)(n_chains + nd);
  u64* plan = (u64*)d_work;
  u64* sums = plan + nc;
  u64* isc = sums + 2 * (size_t)nc;
  u64* ps = isc + (size_t)n_items + 1;
  u64* pd = ps + (size_t)nd + 1;
  u64* partial = pd + (size_t)nd + 1;
  C2pItems it;
  it.lines = (const u64*)d_lines;
  it.line_off = (const u64*)d_line_off;
  it.plan = plan;
  it.n_chains = nc;
  it.n_lines = nd;
  if (!d_out) {
    ScanChainCol col;
    col.lines = (const u64*)d_lines;
    col.col = 0u;
    if ((rc = run_scan_ws(c, col, (u32)nd, ps, partial))) return rc;
    col.col = 1u;
    if ((rc = run_scan_ws(c, col, (u32)nd, pd, partial))) return rc;
    WGA_LAUNCH(k_chain2paf_plan, (nc + 255u) / 256u, WGA_BLOCK, c->stream, d_text, (u64)n_bytes, (const wga_chain_head_dev*)d_heads, nc,
               (const u64*)d_line_off, nd, (const u64*)ps, (const u64*)pd, plan, sums);
    LAUNCH_CHECK();
    ScanC2pItem f;
    f.it = it;
    if ((rc = run_scan_ws(c, f, n_items, isc, partial))) return rc;
    u64 tot = 0;
    RT_CHECK(rt_d2h(&tot, isc + n_items, sizeof tot, c->stream));
    *total_bytes = tot;
    return WGA_OK;
  }
  WGA_LAUNCH(k_chain2paf_fill, (u32)(((u64)n_items + WGA_C2P_ITEMS - 1u) / WGA_C2P_ITEMS), WGA_BLOCK, c->stream, it, (u64)n_items, d_text,
             (u64)n_bytes, (const wga_chain_head_dev*)d_heads, (const u64*)sums, (const u64*)isc, (u64)*total_bytes, d_out);
  LAUNCH_CHECK();
  return WGA_OK;
}

} /* extern "C" */
