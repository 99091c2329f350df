/* capi_maf_frame.inc — K32: the MAF record frames of `paf2maf` and `chain2maf` (wga_k32_maf_frame.h).
 * A part of wga_capi.cpp (included there: one translation unit). */
/* d_work in u64 words, n records: the target heads' bytes [n] | the query heads' bytes [n] | the first bad record [1] | the bytes
 * in front of it [1] | the scan's partials [n / 1024 + 4] */
static size_t maf_frame_work_words(uint64_t n) { return 2 * (size_t)n + 2 + (size_t)(n / 1024u) + 4; }

extern "C" {

uint64_t wga_paf2maf_frame_work_bytes(uint64_t n) { return 8ull * (uint64_t)maf_frame_work_words(n); }

int wga_paf2maf_frame(wga_ctx* c, uint32_t n, const uint8_t* d_names, uint64_t n_name_bytes, const wga_maf_frame_head* d_heads,
                      const wga_cigar_counts* d_counts, const uint64_t* d_t_src_len, const uint64_t* d_q_src_len,
                      const wga_rec_diag* d_diag, void* d_work, uint64_t* d_t_row_off, uint64_t* d_q_row_off, uint64_t* d_rec_off,
                      uint64_t* total_bytes, uint32_t* n_good, uint64_t* good_bytes, uint8_t* d_out) {
  static_assert(sizeof(wga_maf_frame_head) == 88 && sizeof(wga_cigar_counts) == 88 && sizeof(wga_rec_diag) == 24,
                "K32's record layouts");
  int rc = ctx_bind(c);
  if (rc) return rc;
  if (!total_bytes || !n_good || !good_bytes) return fail(WGA_E_INVALID_ARG, "null argument", nullptr);
  if (!d_work) return fail(WGA_E_INVALID_ARG, "d_work null", nullptr);
  /* d_names may be null when no name has a byte: every span is then outside the buffer; d_diag may be null: no record is bad */
  if (n && (!d_heads || !d_counts || !d_t_src_len || !d_q_src_len || !d_t_row_off || !d_q_row_off || !d_rec_off ||
            (n_name_bytes && !d_names)))
    return fail(WGA_E_INVALID_ARG, "null array", nullptr);
  if (!d_out) *total_bytes = 0;
  *n_good = 0, *good_bytes = 0;
  if (n == 0 || (d_out && *total_bytes == 0)) return WGA_OK;
  u64* plan_t = (u64*)d_work;
  u64* plan_q = plan_t + n;
  u64* res = plan_q + n; /* the first bad record, the bytes in front of it */
  u64* partial = res + 2;
  const u8* names = d_names;
  const u64 nnb = d_names ? n_name_bytes : 0u;
  if (!d_out) {
    WGA_LAUNCH(k_maf_frame_plan, (u32)(((u64)n + 255u) / 256u), WGA_BLOCK, c->stream, names, nnb, d_heads, n, plan_t, plan_q);
    LAUNCH_CHECK();
    ScanMafRecs f;
    f.rows.counts = d_counts;
    f.rows.t_src_len = (const u64*)d_t_src_len;
    f.rows.q_src_len = (const u64*)d_q_src_len;
    f.rows.pre_t = f.rows.pre_q = f.rows.post = nullptr;
    f.plan_t = plan_t;
    f.plan_q = plan_q;
    if ((rc = run_scan_ws(c, f, n, (u64*)d_rec_off, partial))) return rc;
    WGA_LAUNCH(k_maf_frame_place, (u32)(((u64)n + 255u) / 256u), WGA_BLOCK, c->stream, f, n, (const u64*)d_rec_off,
               (u64*)d_t_row_off, (u64*)d_q_row_off);
    LAUNCH_CHECK();
    u64 total = 0;
    RT_CHECK(rt_d2h(&total, d_rec_off + n, sizeof total, c->stream));
    *total_bytes = total;
    *n_good = n; /* no diagnostic is read here */
    *good_bytes = total;
    return WGA_OK;
  }
  RT_CHECK(rt_memset(res, 0xFF, sizeof(u64), c->stream));
  WGA_LAUNCH(k_maf_frame_fill, (u32)(((u64)n + 3u) / 4u), WGA_BLOCK, c->stream, names, nnb, d_heads, n, d_diag, (const u64*)plan_t,
             (const u64*)plan_q, (const u64*)d_rec_off, (const u64*)d_q_row_off, (u64)*total_bytes, d_out, res);
  LAUNCH_CHECK();
  WGA_LAUNCH(k_maf_frame_result, 1u, WGA_BLOCK, c->stream, n, (const u64*)d_rec_off, res);
  LAUNCH_CHECK();
  u64 got[2] = {0, 0};
  RT_CHECK(rt_d2h(got, res, sizeof got, c->stream));
  *n_good = got[0] < (u64)n ? (u32)got[0] : n;
  *good_bytes = got[1];
  return WGA_OK;
}

} /* extern "C" */
