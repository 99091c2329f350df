/* capi_chain_heads.inc — K30: the chain heads of `paf2chain` and `maf2chain` (wga_k30_chain_heads.h).
 * A part of wga_capi.cpp (included there: one translation unit). */
/* d_work in u64 words, n records: the plan (a head's bytes) [n] | the scan of the record sizes [n + 1] | the first bad record [1] |
 * the scan's partials [n / 1024 + 4] */
static size_t chain_heads_work_words(uint64_t n) { return 2 * (size_t)n + 2 + (size_t)(n / 1024u) + 4; }

extern "C" {

uint64_t wga_chain_heads_work_bytes(uint64_t n) { return 8ull * (uint64_t)chain_heads_work_words(n); }

int wga_chain_heads(wga_ctx* c, uint32_t n, const uint8_t* d_names, uint64_t n_name_bytes, const wga_maf2paf_head* d_heads,
                    const wga_chain_trim_t* d_trim, const uint64_t* d_nbytes, const wga_rec_diag* d_diag, uint64_t chain_id0,
                    void* d_work, uint64_t* d_data_off, uint64_t* total_bytes, uint32_t* n_good, uint8_t* d_out) {
  static_assert(sizeof(wga_maf2paf_head) == 80 && sizeof(wga_chain_trim_t) == 32 && sizeof(wga_rec_diag) == 24, "K30's record layouts");
  int rc = ctx_bind(c);
  if (rc) return rc;
  if (!total_bytes || !n_good) return fail(WGA_E_INVALID_ARG, "null argument", nullptr);
  if (!d_work) return fail(WGA_E_INVALID_ARG, "d_work null", nullptr);
  /* d_names may be null when no name has a byte: every span is then outside the buffer */
  if (n && (!d_heads || !d_trim || !d_nbytes || !d_diag || !d_data_off || (n_name_bytes && !d_names)))
    return fail(WGA_E_INVALID_ARG, "null array", nullptr);
  if (!d_out) *total_bytes = 0, *n_good = 0;
  if (n == 0 || (d_out && *total_bytes == 0)) return WGA_OK;
  u64* plan = (u64*)d_work;
  u64* rec_off = plan + n;
  u64* first_bad = rec_off + (size_t)n + 1; /* behind the total: the two results come back in one copy */
  u64* partial = first_bad + 1;
  const u8* names = d_names;
  const u64 nnb = d_names ? n_name_bytes : 0u;
  if (!d_out) {
    RT_CHECK(rt_memset(first_bad, 0xFF, sizeof(u64), c->stream));
    WGA_LAUNCH(k_chain_heads_plan, (u32)(((u64)n + 255u) / 256u), WGA_BLOCK, c->stream, names, nnb, d_heads, n, d_trim, d_diag,
               (u64)chain_id0, plan, first_bad);
    LAUNCH_CHECK();
    ScanChainRecs f;
    f.plan = plan;
    f.nbytes = (const u64*)d_nbytes;
    f.n_good = first_bad;
    if ((rc = run_scan_ws(c, f, n, rec_off, partial))) return rc;
    WGA_LAUNCH(k_chain_heads_place, (u32)(((u64)n + 255u) / 256u), WGA_BLOCK, c->stream, n, (const u64*)plan, (const u64*)rec_off,
               (const u64*)first_bad, (u64*)d_data_off);
    LAUNCH_CHECK();
    u64 res[2] = {0, 0}; /* the total, the first bad record */
    RT_CHECK(rt_d2h(res, rec_off + n, sizeof res, c->stream));
    *total_bytes = res[0];
    *n_good = res[1] < (u64)n ? (u32)res[1] : n;
    return WGA_OK;
  }
  const u32 ng = *n_good < n ? *n_good : n;
  if (ng == 0) return WGA_OK;
  WGA_LAUNCH(k_chain_heads_fill, (u32)(((u64)ng + 3u) / 4u), WGA_BLOCK, c->stream, names, nnb, d_heads, ng, d_trim, (u64)chain_id0,
             (const u64*)plan, (const u64*)rec_off, (u64)*total_bytes, d_out);
  LAUNCH_CHECK();
  return WGA_OK;
}

} /* extern "C" */
