/* capi_stat_pairs.inc — K36: stat's merged table (wga_k36_stat_pairs.h): the pairs of a piece with their sums, and the pairs' rows.
 * A part of wga_capi.cpp (included there: one translation unit; run_group, run_sort_u32 and the scan driver stand there). */

/* d_work of K36, n records.  u64 words: K36Hdr [8] | the table [M = group_slots(n)] | the scan of "is its pair's first" [n + 1] | the
 * scan of "is inverted" over the sorted places [n + 1] | the sort's digit counts [C = sort_cnt_words(n)] | the scans' partials
 * [n / 1024 + C / 1024 + 8]; then u32: the pairs' lowest records [n] | start slots, later the records' pairs [n] | the two lists of
 * records without a pair, later the sort's two buffers [n] each | the pairs' first places [n + 2] | the inverted records' values [n] */
struct StatPairsWork {
  K36Hdr* hdr;
  u64 *slots, *gidx, *invsc, *cnt, *partial;
  u32 *rep, *gs, *list[2], *gstart, *inv_val;
  size_t bytes;
};
static StatPairsWork stat_pairs_work(void* d_work, uint64_t n) {
  StatPairsWork W;
  const size_t N = (size_t)n, M = (size_t)group_slots(n), C = sort_cnt_words(n);
  u64* p = (u64*)d_work;
  W.hdr = (K36Hdr*)p, p += 8;
  W.slots = p, p += M;
  W.gidx = p, p += N + 1;
  W.invsc = p, p += N + 1;
  W.cnt = p, p += C;
  W.partial = p, p += N / 1024 + C / 1024 + 8;
  u32* q = (u32*)p;
  W.rep = q, q += N;
  W.gs = q, q += N;
  W.list[0] = q, q += N;
  W.list[1] = q, q += N;
  W.gstart = q, q += N + 2;
  W.inv_val = q, q += N;
  W.bytes = ((size_t)((char*)q - (char*)d_work) + 7u) & ~(size_t)7u;
  return W;
}

extern "C" {

uint64_t wga_stat_pairs_work_bytes(uint64_t n) { return (uint64_t)stat_pairs_work(nullptr, n).bytes; }

int wga_stat_pairs(wga_ctx* c, uint32_t n, const uint8_t* d_names, uint64_t n_name_bytes, const wga_stat_row_head* d_heads,
                   const wga_cigar_counts* d_counts, void* d_work, uint64_t* n_pairs, uint32_t* d_pair_of_rec,
                   const uint32_t* d_inv_in, wga_stat_pair* d_pairs, uint64_t cap_pairs) {
  static_assert(sizeof(wga_stat_pair) == 128 && sizeof(wga_stat_pair_dev) == 128 && sizeof(K36Hdr) == 64, "K36's layouts");
  static_assert(offsetof(wga_stat_pair, sum) == offsetof(wga_stat_pair_dev, sum) &&
                    offsetof(wga_stat_pair, inv_size_bits) == offsetof(wga_stat_pair_dev, inv_size_bits),
                "wga_stat_pair layout");
  int rc = ctx_bind(c);
  if (rc) return rc;
  if (!d_work || !n_pairs) return fail(WGA_E_INVALID_ARG, "null argument", nullptr);
  if (n > 0xFFFFFFF0u) return fail(WGA_E_INVALID_ARG, "more than 0xFFFFFFF0 records", nullptr);
  /* d_names may be null when no name has a byte: every span is then outside the buffer */
  if (n && (!d_heads || !d_counts || (n_name_bytes && !d_names))) return fail(WGA_E_INVALID_ARG, "null array", nullptr);
  const bool second = d_pairs != nullptr || d_pair_of_rec != nullptr;
  const StatPairsWork W = stat_pairs_work(d_work, n);
  const u32 grid = (u32)(((u64)n + 255u) / 256u);
  if (!second) {
    *n_pairs = 0;
    if (n == 0) return WGA_OK;
    StatPairKey key;
    key.names = d_names;
    key.n_name_bytes = d_names ? n_name_bytes : 0u;
    key.heads = d_heads;
    u64 ng = 0;
    if ((rc = run_group(c, key, n, c->stat_pair_hash_bits, &W.hdr->g, W.slots, W.rep, W.gs, W.list, W.gidx, W.partial, &ng))) return rc;
    /* input order within a pair: the stable sort by pair */
    SortStatPairKey sk;
    sk.gs = W.gs;
    int where = 0;
    if ((rc = run_sort_u32(c, sk, n, sort_key_bits(ng), WGA_SORT_MAX_BITS, W.list, W.cnt, W.partial, &where))) return rc;
    const u32* order = W.list[where];
    WGA_LAUNCH(k_stat_pairs_bounds, grid, WGA_BLOCK, c->stream, (u64)n, ng, order, (const u32*)W.gs, W.gstart, W.hdr, (u64)where);
    LAUNCH_CHECK();
    ScanStatPairInv fi;
    fi.order = order;
    fi.counts = d_counts;
    fi.n = n;
    if ((rc = run_scan_ws(c, fi, n, W.invsc, W.partial))) return rc;
    WGA_LAUNCH(k_stat_pairs_inv_vals, grid, WGA_BLOCK, c->stream, (u64)n, order, d_counts, (const u64*)W.invsc, W.inv_val);
    LAUNCH_CHECK();
    RT_CHECK(rt_sync(c->stream));
    *n_pairs = ng;
    return WGA_OK;
  }
  if (n == 0) return WGA_OK;
  if (!d_pairs || !d_pair_of_rec) return fail(WGA_E_INVALID_ARG, "null array", nullptr);
  K36Hdr h;
  RT_CHECK(rt_d2h(&h, W.hdr, sizeof h, c->stream));
  if (h.n != n || h.n_pairs != *n_pairs || *n_pairs == 0 || *n_pairs > n || h.where > 1u)
    return fail(WGA_E_INVALID_ARG, "the counts are not the first call's", nullptr);
  if (cap_pairs < *n_pairs) return fail(WGA_E_TOO_SMALL, "cap_pairs is less than the pairs", nullptr);
  const u64 ng = *n_pairs;
  const u32* order = W.list[h.where];
  wga_stat_pair_dev* pairs = (wga_stat_pair_dev*)d_pairs;
  /* a repeat of the second call on the same outputs: only the fold depends on d_inv_in */
  const u64 filled[2] = {(u64)(uintptr_t)d_pairs, (u64)(uintptr_t)d_pair_of_rec};
  if (h.filled[0] != filled[0] || h.filled[1] != filled[1]) {
    WGA_LAUNCH(k_stat_pairs_of_rec, grid, WGA_BLOCK, c->stream, (u64)n, (const u32*)W.gs, d_pair_of_rec);
    LAUNCH_CHECK();
    WGA_LAUNCH(k_stat_pairs_init, (u32)((ng + 255u) / 256u), WGA_BLOCK, c->stream, (u64)n, ng, order, (const u32*)W.gstart, d_heads,
               pairs);
    LAUNCH_CHECK();
    WGA_LAUNCH(k_stat_pairs_reduce, grid, WGA_BLOCK, c->stream, (u64)n, ng, order, (const u32*)W.gs, (const u32*)W.gstart, d_heads,
               d_counts, pairs);
    LAUNCH_CHECK();
  }
  WGA_LAUNCH(k_stat_pairs_fold, (u32)((ng + 3u) / 4u), WGA_BLOCK, c->stream, (u64)n, ng, (const u32*)W.gstart, (const u64*)W.invsc,
             (const u32*)W.inv_val, d_inv_in, pairs, W.hdr, filled[0], filled[1]);
  LAUNCH_CHECK();
  return WGA_OK;
}

int wga_stat_pair_rows(wga_ctx* c, uint32_t n, const uint8_t* d_names, uint64_t n_name_bytes, const wga_stat_row_head* d_heads,
                       const wga_cigar_counts* d_sums, const uint32_t* d_inv_bits, void* d_work, uint64_t* d_row_off,
                       uint64_t* total_bytes, uint8_t* d_out) {
  int rc = ctx_bind(c);
  if (rc) return rc;
  if (!total_bytes) return fail(WGA_E_INVALID_ARG, "null argument", nullptr);
  if (!d_work) return fail(WGA_E_INVALID_ARG, "d_work null", nullptr);
  if (n > 0xFFFFFFF0u) return fail(WGA_E_INVALID_ARG, "more than 0xFFFFFFF0 rows", nullptr);
  if (n && (!d_heads || !d_sums || !d_inv_bits || !d_row_off || (n_name_bytes && !d_names)))
    return fail(WGA_E_INVALID_ARG, "null array", nullptr);
  if (!d_out) *total_bytes = 0;
  if (n == 0 || (d_out && *total_bytes == 0)) return WGA_OK;
  StatPairRowsFmt f;
  f.names = d_names;
  f.n_name_bytes = d_names ? n_name_bytes : 0u;
  f.heads = d_heads;
  f.counts = d_sums;
  f.inv_bits = d_inv_bits;
  f.plan = (u64*)d_work; /* the layout of run_record_rows: the plan [n] | the scan's partials */
  f.n_rec = n;
  if (d_out) return run_text_items_fill(c, f, n, (const u64*)d_row_off, (u64)*total_bytes, d_out);
  const StatPairRowSrc src = f;
  WGA_LAUNCH(k_stat_pair_rows_plan, (u32)(((u64)n + 255u) / 256u), WGA_BLOCK, c->stream, src, n, (u64*)d_work);
  LAUNCH_CHECK();
  if ((rc = run_scan_ws(c, ScanItems<StatPairRowsFmt>{f}, n, (u64*)d_row_off, (u64*)d_work + n))) return rc;
  u64 tot = 0;
  RT_CHECK(rt_d2h(&tot, d_row_off + n, sizeof tot, c->stream));
  *total_bytes = tot;
  return WGA_OK;
}

} /* extern "C" */
