/* capi_maf_index.inc — K35: maf-index on the device (wga_k35_maf_index.h): block offsets, name groups, the JSON interval text.
 * A part of wga_capi.cpp (included there: one translation unit). */

/* d_work of K35, n = n_lines.  u64 words: the newline pass's header [2] | K35Hdr [8] | the lines' scan P [n + 1] | the blocks'
 * offsets [n + 2] | the table [M] | the scan of "is its group's first" [n + 1] | the intervals' scan [n + 1] | the intervals [4 n] |
 * the sort's digit counts [sort_cnt_words(n)] | the scans' partials; then u32: the newlines' positions [n] | the s-lines' lines [n]
 * | their groups' first s-lines [n] | start slots, later the s-lines' groups [n] | the two lists of s-lines without a group, later
 * the sort's two buffers [n] each | the groups' first places [n + 1] */
struct MafIdxWork {
  K24Hdr* nl_hdr;
  K35Hdr* hdr;
  u64 *P, *blk_off, *slots, *gidx, *isc, *cnt, *partial;
  MafIdxIvl* ivl;
  u32 *nl_pos, *sl_line, *rep, *start, *list[2], *gstart;
  size_t bytes;
};
static MafIdxWork maf_index_work(void* d_work, uint64_t n) {
  MafIdxWork W;
  const size_t N = (size_t)n, M = (size_t)paf_pair_slots(n), C = sort_cnt_words(n);
  u64* p = (u64*)d_work;
  W.nl_hdr = (K24Hdr*)p, p += 2;
  W.hdr = (K35Hdr*)p, p += 8;
  W.P = p, p += N + 1;
  W.blk_off = p, p += N + 2;
  W.slots = p, p += M;
  W.gidx = p, p += N + 1;
  W.isc = p, p += N + 1;
  W.ivl = (MafIdxIvl*)p, p += 4 * N;
  W.cnt = p, p += C;
  W.partial = p, p += N / 1024 + C / 1024 + 8;
  u32* q = (u32*)p;
  W.nl_pos = q, q += N;
  W.sl_line = q, q += N;
  W.rep = q, q += N;
  W.start = q, q += N;
  W.list[0] = q, q += N;
  W.list[1] = q, q += N;
  W.gstart = q, q += N + 2;
  W.bytes = (size_t)((char*)q - (char*)d_work);
  return W;
}

extern "C" {

uint64_t wga_maf_index_work_bytes(uint64_t n_lines) { return (uint64_t)maf_index_work(nullptr, n_lines).bytes; }

int wga_maf_index(wga_ctx* c, const uint8_t* d_text, uint64_t n_bytes, const wga_maf_line* d_lines, uint64_t n_lines, uint32_t skip,
                  uint64_t base, uint64_t carry_offset, void* d_work, uint64_t* n_names, uint64_t* n_blocks, uint64_t* n_slines,
                  uint64_t* text_bytes, uint64_t* first_dup_line, uint64_t* first_conflict_line, uint64_t* next_offset,
                  wga_maf_index_name* d_names, uint8_t* d_out) {
  int rc = ctx_bind(c);
  if (rc) return rc;
  static_assert(sizeof(wga_maf_index_name) == 48 && sizeof(wga_maf_index_name) == sizeof(wga_maf_index_name_dev), "wga_maf_index_name layout");
  static_assert(sizeof(MafIdxIvl) == 32 && sizeof(K35Hdr) == 64, "K35 work layout");
  if (!d_work || !n_names || !n_blocks || !n_slines || !text_bytes || !first_dup_line || !first_conflict_line || !next_offset)
    return fail(WGA_E_INVALID_ARG, "null argument", nullptr);
  if (skip != 0u && skip != 2u) return fail(WGA_E_INVALID_ARG, "skip: 0, or 2 for a piece behind the dummy line", nullptr);
  if (n_lines >= 0xFFFFFFFFull || n_bytes >= 0xFFFFFFF0ull) return fail(WGA_E_INVALID_ARG, "a text within wga_maf_split's limits", nullptr);
  if (n_lines && (!d_text || !d_lines || n_bytes == 0)) return fail(WGA_E_INVALID_ARG, "null array", nullptr);
  const u32 n = (u32)n_lines;
  const MafIdxWork W = maf_index_work(d_work, n_lines);
  const wga_maf_line_dev* lines = (const wga_maf_line_dev*)d_lines;
  const bool fill = d_names != nullptr || d_out != nullptr;
  if (!fill) {
    *n_names = *n_blocks = *n_slines = *text_bytes = 0;
    *first_dup_line = *first_conflict_line = WGA_NONE;
    *next_offset = carry_offset;
    if (n == 0) return WGA_OK;
    const u64* n_nl_p = nullptr;
    u64* lpartial = nullptr; /* the newline pass's own, in the context scratch: the scans here keep theirs in d_work */
    if ((rc = paf_newline_list(c, d_text, n_bytes, n, W.nl_pos, W.nl_hdr, &n_nl_p, &lpartial))) return rc;
    RT_CHECK(rt_memset(W.hdr, 0xFF, 3 * sizeof(u64), c->stream));
    RT_CHECK(rt_memset(&W.hdr->last_is_s, 0, 5 * sizeof(u64), c->stream));
    const u32 gl = (n + 255u) / 256u;
    WGA_LAUNCH(k_maf_index_lines, gl, WGA_BLOCK, c->stream, lines, (u64)n, W.hdr);
    LAUNCH_CHECK();
    ScanMafIdxLine fl;
    fl.lines = lines;
    if ((rc = run_scan_ws(c, fl, n, W.P, W.partial))) return rc;
    WGA_LAUNCH(k_maf_index_offsets, gl, WGA_BLOCK, c->stream, lines, (u64)n, (u64)n_bytes, n_nl_p, (const u32*)W.nl_pos,
               (const u64*)W.P, (u64)skip, (u64)base, (u64)carry_offset, W.blk_off, W.sl_line);
    LAUNCH_CHECK();
    K35Hdr h;
    u64 tot = 0;
    RT_CHECK(rt_d2h(&h, W.hdr, sizeof h, c->stream));
    RT_CHECK(rt_d2h(&tot, W.P + n, sizeof tot, c->stream));
    if (h.first_fallback != WGA_NONE) return fail(WGA_E_FALLBACK, "the table holds a WGA_MAF_FALLBACK line: the piece is the host reader's", nullptr);
    const u64 ns = tot & 0xFFFFFFFFull, nb = tot >> 32;
    if (ns > n || nb > ns) return fail(WGA_E_HIP, "the lines' scan is not a scan", nullptr);
    /* the last anchor: behind the line that ended the last run — or, for a run without one, where that run's block starts */
    RT_CHECK(rt_d2h(next_offset, W.blk_off + (nb - (h.last_is_s && nb ? 1u : 0u)), sizeof(u64), c->stream));
    *n_blocks = nb;
    *n_slines = ns;
    if (ns == 0) return WGA_OK;
    /* the groups (as wga_paf_pairs) */
    const u64 M = paf_pair_slots(ns);
    const u32 slot_mask = (u32)(M - 1u);
    const unsigned bits = c->maf_index_hash_bits;
    const u64 hash_mask = bits >= 64u ? ~0ull : (1ull << bits) - 1ull;
    const u32 gs_grid = (u32)((ns + 255u) / 256u);
    RT_CHECK(rt_memset(W.slots, 0xFF, (size_t)M * sizeof(u64), c->stream));
    WGA_LAUNCH(k_maf_index_init, gs_grid, WGA_BLOCK, c->stream, d_text, lines, (const u32*)W.sl_line, ns, hash_mask, slot_mask, W.start,
               W.rep, W.list[0]);
    LAUNCH_CHECK();
    u64 m = ns;
    for (u64 r = 0; m; r++) { /* every round gives the lowest s-line of each start slot's class a group, or steps over a taken slot */
      if (m > ns || r > 2u * M + 64u) return fail(WGA_E_HIP, "the name table did not settle", nullptr);
      const u32 g = (u32)((m + 255u) / 256u);
      WGA_LAUNCH(k_maf_index_claim, g, WGA_BLOCK, c->stream, (const u32*)W.list[r & 1u], m, r, slot_mask, (const u32*)W.start, W.slots,
                 W.hdr);
      LAUNCH_CHECK();
      WGA_LAUNCH(k_maf_index_settle, g, WGA_BLOCK, c->stream, d_text, lines, (const u32*)W.sl_line, (const u32*)W.list[r & 1u], m, r,
                 slot_mask, (const u32*)W.start, (const u64*)W.slots, W.rep, W.list[(r + 1u) & 1u], W.hdr);
      LAUNCH_CHECK();
      RT_CHECK(rt_d2h(&m, &W.hdr->cnt[(r + 1u) & 1u], sizeof m, c->stream));
    }
    ScanMafIdxRep fr;
    fr.rep = W.rep;
    if ((rc = run_scan_ws(c, fr, (u32)ns, W.gidx, W.partial))) return rc;
    u64 ng = 0;
    RT_CHECK(rt_d2h(&ng, W.gidx + ns, sizeof ng, c->stream));
    if (ng == 0 || ng > ns) return fail(WGA_E_HIP, "the groups' scan is not a scan", nullptr);
    /* file order within a group: the stable sort by group */
    u32* const gs = W.start; /* the start slots are done with */
    WGA_LAUNCH(k_maf_index_groups, gs_grid, WGA_BLOCK, c->stream, ns, (const u32*)W.rep, (const u64*)W.gidx, gs, W.list[0]);
    LAUNCH_CHECK();
    SortMafIdxKey key;
    key.gs = gs;
    int where = 0;
    if ((rc = run_sort_u32(c, key, (u32)ns, sort_key_bits(ng), c->maf_index_sort_bits, W.list, W.cnt, W.partial, &where))) return rc;
    WGA_LAUNCH(k_maf_index_items, gs_grid, WGA_BLOCK, c->stream, lines, (const u32*)W.sl_line, ns, ng, (const u32*)W.list[where],
               (const u32*)gs, (const u64*)W.P, (const u64*)W.blk_off, W.ivl, W.gstart, W.hdr, (u64)where);
    LAUNCH_CHECK();
    MafIdxFmt f;
    f.ivl = W.ivl;
    f.n_rec = 1u;
    if ((rc = run_scan_ws(c, ScanItems<MafIdxFmt>{f}, (u32)ns, W.isc, W.partial))) return rc;
    RT_CHECK(rt_d2h(&tot, W.isc + ns, sizeof tot, c->stream));
    RT_CHECK(rt_d2h(&h, W.hdr, sizeof h, c->stream));
    *n_names = ng;
    *text_bytes = tot;
    *first_dup_line = h.first_dup;
    *first_conflict_line = h.first_conflict;
    return WGA_OK;
  }
  if (n == 0 || *n_slines == 0) return WGA_OK;
  if (*n_names == 0 || *n_names > *n_slines || *n_slines > n_lines || *text_bytes == 0)
    return fail(WGA_E_INVALID_ARG, "the counts are not the first call's", nullptr);
  if (!d_names || !d_out) return fail(WGA_E_INVALID_ARG, "null array", nullptr);
  const u32 ns = (u32)*n_slines;
  WGA_LAUNCH(k_maf_index_names, (u32)((*n_names + 256u) / 256u), WGA_BLOCK, c->stream, lines, (const u32*)W.sl_line, (u64)ns,
             (u64)*n_names, (const u32*)W.list[0], (const u32*)W.list[1], (const K35Hdr*)W.hdr, (const u32*)W.gstart,
             (const u64*)W.isc, (wga_maf_index_name_dev*)d_names);
  LAUNCH_CHECK();
  MafIdxFmt f;
  f.ivl = W.ivl;
  f.n_rec = 1u;
  return run_text_items_fill(c, f, ns, (const u64*)W.isc, (u64)*text_bytes, d_out);
}

} /* extern "C" */
