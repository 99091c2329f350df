/* capi_text.inc — K8 / K9 / K13 / K14 / K15 / K17 / K18 / K23 / K24: text in, text out (tokenisers, line splitters, FASTA pool, BGZF, BED
 * lines, the PAF line filter and its pair sums).
 * A part of wga_capi.cpp (included there: one translation unit). */
/* K13 / K14 / K23: the two delimiter lists of a text (count, scan, fill over 4 KB blocks) in the context scratch, with `tail`
 * bytes of the caller's own behind them (tail_per_256_lines for every 256 lines or part of them, plus tail_fixed).
 * MODE 0 = PAF (tab, newline, '"', CR), 1 = MAF and chain (newline, white space, bytes >= 0x80). */
struct DelimLists {
  u64 n_delims = 0, n_newlines = 0, n_lines = 0;
  u64* delims = nullptr;
  u64* nl_idx = nullptr;
  void* tail = nullptr;
};
template <int MODE>
static int delim_lists(wga_ctx* c, const uint8_t* d_text, uint64_t n_bytes, bool fill, size_t tail_per_256_lines,
                       size_t tail_fixed, DelimLists* L) {
  int rc;
  const u32 nb = (u32)((n_bytes + 4095u) / 4096u);
  const size_t head = ((size_t)nb + 1 + (size_t)nb / 1024 + 4) * sizeof(u64);
  u64 tot = 0;
  void* ws = nullptr;
  if ((rc = ctx_scratch(c, head, &ws))) return rc;
  size_t lists = 0;
  for (int attempt = 0; attempt < 2; attempt++) {
    u64* blk = (u64*)c->scratch.mem;
    WGA_LAUNCH((k_paf_delims<false, MODE>), nb, WGA_BLOCK, c->stream, d_text, (u64)n_bytes, blk, (const u64*)nullptr,
               (u64*)nullptr, (u64*)nullptr);
    LAUNCH_CHECK();
    /* exclusive scan of the block counts in place (k_scan_final reads its four values, then writes them) */
    ScanPlain f;
    f.in = blk;
    if ((rc = run_scan_ws(c, f, nb, blk, blk + nb + 1))) return rc;
    RT_CHECK(rt_d2h(&tot, blk + nb, sizeof(u64), c->stream));
    /* the two lists follow the block offsets; their sizes are only known now: growing the arena
     * drops its contents, so the count pass is repeated once */
    lists = ((size_t)(tot & 0xFFFFFFFFull) + (size_t)(tot >> 32) + 2) * sizeof(u64);
    const size_t want = head + lists + ((size_t)(tot >> 32) / 256 + 2) * tail_per_256_lines + tail_fixed;
    if (c->scratch.cap >= want) break;
    if ((rc = ctx_scratch(c, want, &ws))) return rc;
  }
  L->n_delims = tot & 0xFFFFFFFFull, L->n_newlines = tot >> 32;
  u8 last = 0;
  RT_CHECK(rt_d2h(&last, d_text + n_bytes - 1, 1, c->stream));
  L->n_lines = L->n_newlines + (last != (u8)0x0A ? 1 : 0);
  L->delims = (u64*)((char*)c->scratch.mem + head);
  L->nl_idx = L->delims + L->n_delims + 1;
  L->tail = (char*)c->scratch.mem + head + lists;
  if (!fill) return WGA_OK;
  WGA_LAUNCH((k_paf_delims<true, MODE>), nb, WGA_BLOCK, c->stream, d_text, (u64)n_bytes, (u64*)nullptr,
             (const u64*)c->scratch.mem, L->delims, L->nl_idx);
  LAUNCH_CHECK();
  return WGA_OK;
}

/* K13 / K14 driver: the lists, then one thread per line.  MODE 0 = PAF (wga_paf_line), 1 = MAF (wga_maf_line). */
template <int MODE>
static int split_lines(wga_ctx* c, const uint8_t* d_text, uint64_t n_bytes, uint64_t* n_lines, void* d_lines,
                       uint64_t cap_lines) {
  int rc = ctx_bind(c);
  if (rc) return rc;
  if (!n_lines) return fail(WGA_E_INVALID_ARG, "n_lines null", nullptr);
  *n_lines = 0;
  if (n_bytes == 0) return WGA_OK;
  if (!d_text) return fail(WGA_E_INVALID_ARG, "d_text null", nullptr);
  if (n_bytes >= 0xFFFFFFFFull) return fail(WGA_E_INVALID_ARG, "text of 4 GiB or more: split it at line ends", nullptr);
  DelimLists L;
  if ((rc = delim_lists<MODE>(c, d_text, n_bytes, d_lines != nullptr, 0, 0, &L))) return rc;
  *n_lines = L.n_lines;
  if (!d_lines) return WGA_OK;
  if (cap_lines < *n_lines) return fail(WGA_E_TOO_SMALL, "d_lines too small", nullptr);
  if (MODE == 0) {
    WGA_LAUNCH(k_paf_fields, (u32)((*n_lines + 255u) / 256u), WGA_BLOCK, c->stream, d_text, (u64)n_bytes,
               (u64)*n_lines, L.n_newlines, L.n_delims, (const u64*)L.delims, (const u64*)L.nl_idx, (wga_paf_line_dev*)d_lines);
  } else {
    WGA_LAUNCH(k_maf_lines, (u32)((*n_lines + 255u) / 256u), WGA_BLOCK, c->stream, d_text, (u64)n_bytes,
               (u64)*n_lines, L.n_newlines, L.n_delims, (const u64*)L.delims, (const u64*)L.nl_idx, (wga_maf_line_dev*)d_lines);
  }
  LAUNCH_CHECK();
  return WGA_OK;
}

/* What the count calls of K24's filter and of K29's two entries (capi_paf_fix.inc) start with: the newline list of the text at
 * nl_pos[n] and the first line with a byte >= 0x80 in *hdr (reset here).  The scratch holds the text blocks' newline counts,
 * scanned in place (+ total), that scan's partials and room for the partials of scans over up to n values (*partial);
 * *n_nl_p = the device's count of newlines (the line kernels read it). */
static int paf_newline_list(wga_ctx* c, const uint8_t* d_text, uint64_t n_bytes, u32 n, u32* nl_pos, K24Hdr* hdr, const u64** n_nl_p,
                            u64** partial) {
  int rc;
  const u32 nb = (u32)((n_bytes + 4095u) / 4096u);
  void* ws = nullptr;
  if ((rc = ctx_scratch(c, ((size_t)nb + 1 + (size_t)nb / 1024 + 4 + (size_t)n / 1024 + 4) * sizeof(u64), &ws))) return rc;
  u64* blk = (u64*)ws;
  u64* bpartial = blk + nb + 1;
  *partial = bpartial + (size_t)nb / 1024 + 4;
  *n_nl_p = blk + nb;
  RT_CHECK(rt_memset(hdr, 0xFF, sizeof(K24Hdr), c->stream));
  WGA_LAUNCH(k_paf_newlines<false>, nb, WGA_BLOCK, c->stream, d_text, (u64)n_bytes, blk, (const u64*)nullptr, (u32*)nullptr, (u64)0,
             (K24Hdr*)nullptr);
  LAUNCH_CHECK();
  ScanPlain f;
  f.in = blk;
  if ((rc = run_scan_ws(c, f, nb, blk, bpartial))) return rc;
  u64 n_nl = 0;
  u8 last = 0;
  RT_CHECK(rt_d2h(&n_nl, blk + nb, sizeof n_nl, c->stream));
  RT_CHECK(rt_d2h(&last, d_text + n_bytes - 1, 1, c->stream));
  if (n_nl + (last != (u8)0x0A ? 1u : 0u) != (u64)n) return fail(WGA_E_INVALID_ARG, "n_lines is not this text's", nullptr);
  WGA_LAUNCH(k_paf_newlines<true>, nb, WGA_BLOCK, c->stream, d_text, (u64)n_bytes, (u64*)nullptr, (const u64*)blk, nl_pos, (u64)n, hdr);
  LAUNCH_CHECK();
  return WGA_OK;
}

extern "C" {

int wga_cigar_tokenise(wga_ctx* c, uint32_t n, const uint8_t* d_text, const uint64_t* d_text_off,
                       uint64_t* d_op_cnt, wga_tok_err* d_err, uint32_t* d_ops,
                       const uint64_t* d_op_off) {
  int rc = ctx_bind(c);
  if (rc) return rc;
  if (n == 0) return WGA_OK;
  if (!d_text || !d_text_off) return fail(WGA_E_INVALID_ARG, "null array", nullptr);
  if (d_ops && !d_op_off) return fail(WGA_E_INVALID_ARG, "d_op_off null", nullptr);
  static_assert(sizeof(wga_tok_err) == sizeof(wga_tok_err_dev), "wga_tok_err layout");
  WGA_LAUNCH(k_cigar_tokenise, (n + 3u) / 4u, WGA_BLOCK, c->stream, n, d_text, (const u64*)d_text_off,
             (const u64*)d_text_off + 1, (u64*)d_op_cnt, (wga_tok_err_dev*)d_err, d_ops, (const u64*)d_op_off);
  LAUNCH_CHECK();
  return WGA_OK;
}

int wga_cigar_tokenise_spans(wga_ctx* c, uint32_t n, const uint8_t* d_text, const uint64_t* d_beg,
                             const uint64_t* d_end, uint64_t* d_op_cnt, wga_tok_err* d_err, uint32_t* d_ops,
                             const uint64_t* d_op_off) {
  int rc = ctx_bind(c);
  if (rc) return rc;
  if (n == 0) return WGA_OK;
  if (!d_text || !d_beg || !d_end) return fail(WGA_E_INVALID_ARG, "null array", nullptr);
  if (d_ops && !d_op_off) return fail(WGA_E_INVALID_ARG, "d_op_off null", nullptr);
  WGA_LAUNCH(k_cigar_tokenise, (n + 3u) / 4u, WGA_BLOCK, c->stream, n, d_text, (const u64*)d_beg,
             (const u64*)d_end, (u64*)d_op_cnt, (wga_tok_err_dev*)d_err, d_ops, (const u64*)d_op_off);
  LAUNCH_CHECK();
  return WGA_OK;
}

int wga_paf_split(wga_ctx* c, const uint8_t* d_text, uint64_t n_bytes, uint64_t* n_lines, wga_paf_line* d_lines,
                  uint64_t cap_lines) {
  static_assert(sizeof(wga_paf_line) == sizeof(wga_paf_line_dev), "wga_paf_line layout");
  return split_lines<0>(c, d_text, n_bytes, n_lines, (void*)d_lines, cap_lines);
}

int wga_maf_split(wga_ctx* c, const uint8_t* d_text, uint64_t n_bytes, uint64_t* n_lines, wga_maf_line* d_lines,
                  uint64_t cap_lines) {
  static_assert(sizeof(wga_maf_line) == sizeof(wga_maf_line_dev), "wga_maf_line layout");
  return split_lines<1>(c, d_text, n_bytes, n_lines, (void*)d_lines, cap_lines);
}

/* d_work of K24's filter in u64 words: header [2] | the scan of (bytes | kept << 32) [n + 1] | the kept lines' places [n + 1] |
 * their sources [n] (the scan's input before that) | the newlines' positions, u32 [n] */
uint64_t wga_paf_filter_work_bytes(uint64_t n_lines) { return 8ull * (3ull * n_lines + 4ull + (n_lines + 1ull) / 2ull); }

int wga_paf_filter(wga_ctx* c, const uint8_t* d_text, uint64_t n_bytes, const wga_paf_line* d_lines, uint64_t n_lines,
                   const wga_paf_filter_params* params, void* d_work, uint64_t* text_bytes, uint64_t* n_kept,
                   uint64_t* first_inexact_line, uint8_t* d_out) {
  int rc = ctx_bind(c);
  if (rc) return rc;
  static_assert(sizeof(wga_paf_filter_params) == 32 && sizeof(wga_paf_filter_params) == sizeof(wga_paf_filter_params_dev),
                "K24 params layout");
  if (!params || !text_bytes || !n_kept || !first_inexact_line) return fail(WGA_E_INVALID_ARG, "null argument", nullptr);
  if (n_lines >= 0xFFFFFFFFull || n_bytes >= 0xFFFFFFF0ull) return fail(WGA_E_INVALID_ARG, "a text within wga_paf_split's limits", nullptr);
  if (n_lines && (!d_text || !d_lines || !d_work || n_bytes == 0)) return fail(WGA_E_INVALID_ARG, "null array", nullptr);
  if (params->d_pair_keep && !params->d_pair_of_line) return fail(WGA_E_INVALID_ARG, "d_pair_keep without d_pair_of_line", nullptr);
  const u32 n = (u32)n_lines;
  K24Hdr* hdr = (K24Hdr*)d_work;
  u64* P = (u64*)d_work + 2;
  u64* koff = P + n + 1u;
  u64* ksrc = koff + n + 1u;
  u32* nl_pos = (u32*)(ksrc + n);
  if (!d_out) {
    *text_bytes = 0;
    *n_kept = 0;
    *first_inexact_line = WGA_NONE;
    if (n == 0) return WGA_OK;
    const u64* n_nl_p = nullptr;
    u64* lpartial = nullptr;
    if ((rc = paf_newline_list(c, d_text, n_bytes, n, nl_pos, hdr, &n_nl_p, &lpartial))) return rc;
    wga_paf_filter_params_dev Pd;
    Pd.min_block_size = params->min_block_size;
    Pd.min_query_size = params->min_query_size;
    Pd.pair_of_line = params->d_pair_of_line;
    Pd.pair_keep = params->d_pair_keep;
    WGA_LAUNCH(k_paf_filter_lines, (n + 255u) / 256u, WGA_BLOCK, c->stream, d_text, (u64)n_bytes, (u64)n, n_nl_p,
               (const u32*)nl_pos, (const wga_paf_line_dev*)d_lines, Pd, ksrc, hdr);
    LAUNCH_CHECK();
    ScanPlain f;
    f.in = ksrc;
    if ((rc = run_scan_ws(c, f, n, P, lpartial))) return rc;
    WGA_LAUNCH(k_paf_filter_compact, (n + 255u) / 256u, WGA_BLOCK, c->stream, (u64)n, (const u32*)nl_pos, (const u64*)P, koff, ksrc);
    LAUNCH_CHECK();
    u64 tot = 0;
    K24Hdr h;
    RT_CHECK(rt_d2h(&tot, P + n, sizeof tot, c->stream));
    RT_CHECK(rt_d2h(&h, hdr, sizeof h, c->stream));
    *n_kept = tot >> 32;
    *first_inexact_line = h.first_inexact;
    *text_bytes = h.first_inexact == WGA_NONE ? tot & 0xFFFFFFFFull : 0u;
    return WGA_OK;
  }
  if (n == 0 || *text_bytes == 0) return WGA_OK;
  if (*n_kept == 0 || *n_kept > n_lines || *text_bytes > n_bytes + 1u) return fail(WGA_E_INVALID_ARG, "the counts are not the first call's", nullptr);
  if (((uintptr_t)d_out & 15u) != 0) return fail(WGA_E_INVALID_ARG, "d_out must be 16-byte aligned", nullptr);
  const u64 tiles = (*text_bytes + WGA_PAF_FILTER_TILE - 1u) / WGA_PAF_FILTER_TILE;
  WGA_LAUNCH(k_paf_filter_fill, (u32)tiles, WGA_BLOCK, c->stream, d_text, (const u64*)koff, (const u64*)ksrc, (u32)*n_kept,
             (u64)*text_bytes, d_out);
  LAUNCH_CHECK();
  return WGA_OK;
}

/* d_work of K24's pairs in u64 words: header [2] | the table [M] | sums [n] | the scan of "is a representative" [n + 1] | then u32:
 * representatives [n] | start slots [n] | the two lists of lines without a pair [n] each */
static uint64_t paf_pair_slots(uint64_t n_lines) {
  uint64_t m = 16;
  while (m < 2 * n_lines && m < (1ull << 32)) m <<= 1;
  return m;
}
uint64_t wga_paf_pairs_work_bytes(uint64_t n_lines) {
  return 8ull * (2ull + paf_pair_slots(n_lines) + 2ull * n_lines + 1ull) + 16ull * n_lines;
}

int wga_paf_pairs(wga_ctx* c, const uint8_t* d_text, uint64_t n_bytes, const wga_paf_line* d_lines, uint64_t n_lines, void* d_work,
                  uint64_t* n_pairs, uint32_t* d_pair_of_line, wga_paf_pair* d_pairs, uint64_t cap_pairs) {
  int rc = ctx_bind(c);
  if (rc) return rc;
  static_assert(sizeof(wga_paf_pair) == 40 && sizeof(wga_paf_pair) == sizeof(wga_paf_pair_dev), "wga_paf_pair layout");
  if (!n_pairs) return fail(WGA_E_INVALID_ARG, "n_pairs null", nullptr);
  if (n_lines >= 0xFFFFFFFFull || n_bytes >= 0xFFFFFFF0ull) return fail(WGA_E_INVALID_ARG, "a text within wga_paf_split's limits", nullptr);
  if (n_lines && (!d_text || !d_lines || !d_work)) return fail(WGA_E_INVALID_ARG, "null array", nullptr);
  const u32 n = (u32)n_lines;
  const u64 M = paf_pair_slots(n_lines);
  const u32 slot_mask = (u32)(M - 1u);
  K24PairHdr* hdr = (K24PairHdr*)d_work;
  u64* slots = (u64*)d_work + 2;
  u64* sum = slots + M;
  u64* pidx = sum + n;
  u32* rep = (u32*)(pidx + n + 1u);
  u32* start = rep + n;
  u32* list[2] = {start + n, start + 2u * (size_t)n};
  const bool fill = d_pair_of_line != nullptr || d_pairs != nullptr;
  if (!fill) {
    *n_pairs = 0;
    if (n == 0) return WGA_OK;
    const unsigned bits = c->paf_pair_hash_bits;
    const u64 hash_mask = bits >= 64u ? ~0ull : (1ull << bits) - 1ull;
    RT_CHECK(rt_memset(hdr, 0, sizeof(K24PairHdr), c->stream));
    RT_CHECK(rt_memset(slots, 0xFF, (size_t)M * sizeof(u64), c->stream));
    const wga_paf_line_dev* lines = (const wga_paf_line_dev*)d_lines;
    WGA_LAUNCH(k_paf_pairs_init, (n + 255u) / 256u, WGA_BLOCK, c->stream, d_text, lines, (u64)n, hash_mask, slot_mask, start, rep,
               sum, list[0], hdr);
    LAUNCH_CHECK();
    u64 m = 0;
    RT_CHECK(rt_d2h(&m, &hdr->cnt[0], sizeof m, c->stream));
    for (u64 r = 0; m; r++) { /* every round gives the lowest line of each start slot's class a pair, or steps over a taken slot */
      if (m > n || r > 2u * M + 64u) return fail(WGA_E_HIP, "the pair table did not settle", nullptr);
      const u32 g = (u32)((m + 255u) / 256u);
      WGA_LAUNCH(k_paf_pairs_claim, g, WGA_BLOCK, c->stream, (const u32*)list[r & 1u], m, r, slot_mask, (const u32*)start, slots, hdr);
      LAUNCH_CHECK();
      WGA_LAUNCH(k_paf_pairs_settle, g, WGA_BLOCK, c->stream, d_text, lines, (const u32*)list[r & 1u], m, r, slot_mask,
                 (const u32*)start, (const u64*)slots, rep, sum, list[(r + 1u) & 1u], hdr);
      LAUNCH_CHECK();
      RT_CHECK(rt_d2h(&m, &hdr->cnt[(r + 1u) & 1u], sizeof m, c->stream));
    }
    ScanPairRep f;
    f.rep = rep;
    if ((rc = run_scan(c, f, n, pidx))) return rc;
    u64 np = 0;
    RT_CHECK(rt_d2h(&np, pidx + n, sizeof np, c->stream));
    *n_pairs = np;
    return WGA_OK;
  }
  if (n == 0) return WGA_OK;
  if (!d_pair_of_line || (*n_pairs && !d_pairs)) return fail(WGA_E_INVALID_ARG, "null array", nullptr);
  if (cap_pairs < *n_pairs) return fail(WGA_E_TOO_SMALL, "d_pairs too small", nullptr);
  WGA_LAUNCH(k_paf_pairs_emit, (n + 255u) / 256u, WGA_BLOCK, c->stream, (const wga_paf_line_dev*)d_lines, (u64)n, (const u32*)rep,
             (const u64*)sum, (const u64*)pidx, (u32*)d_pair_of_line, (wga_paf_pair_dev*)d_pairs);
  LAUNCH_CHECK();
  return WGA_OK;
}

int wga_chain_split(wga_ctx* c, const uint8_t* d_text, uint64_t n_bytes, uint64_t* n_chains, uint64_t* n_data_lines,
                    uint32_t* status, uint64_t* first_bad_line, wga_chain_head* d_heads, uint64_t cap_chains, uint64_t* d_lines,
                    uint64_t cap_lines, uint64_t* d_line_off) {
  static_assert(sizeof(wga_chain_head) == sizeof(wga_chain_head_dev) && sizeof(wga_chain_head) == 96, "wga_chain_head layout");
  int rc = ctx_bind(c);
  if (rc) return rc;
  if (!n_chains || !n_data_lines || !status || !first_bad_line) return fail(WGA_E_INVALID_ARG, "null count", nullptr);
  *n_chains = *n_data_lines = 0;
  *status = WGA_CHAIN_OK;
  *first_bad_line = WGA_NONE;
  const bool fill = d_heads != nullptr || d_lines != nullptr || d_line_off != nullptr;
  if (fill && !d_line_off) return fail(WGA_E_INVALID_ARG, "d_line_off null", nullptr);
  if (n_bytes == 0) { /* an empty file: no chain */
    static const u64 zero = 0;
    if (fill) RT_CHECK(rt_h2d(d_line_off, &zero, sizeof zero, c->stream));
    return WGA_OK;
  }
  if (!d_text) return fail(WGA_E_INVALID_ARG, "d_text null", nullptr);
  if (n_bytes >= 0xFFFFFFF0ull) return fail(WGA_E_INVALID_ARG, "text of 4 GiB or more: the host reader takes it", nullptr);
  /* behind the lists: the line blocks' counts (then offsets, + total) | scan partials | the first bad line */
  DelimLists L;
  if ((rc = delim_lists<1>(c, d_text, n_bytes, true, 16, 128, &L))) return rc;
  const u32 nlb = (u32)((L.n_lines + 255u) / 256u);
  u64* blk = (u64*)L.tail;
  u64* partial = blk + nlb + 1;
  u64* first_bad = partial + (size_t)nlb / 1024 + 4;
  WGA_LAUNCH(k_chain_kinds, nlb, WGA_BLOCK, c->stream, d_text, (u64)n_bytes, L.n_lines, L.n_newlines, (const u64*)L.delims,
             (const u64*)L.nl_idx, blk);
  LAUNCH_CHECK();
  ScanPlain f;
  f.in = blk;
  if ((rc = run_scan_ws(c, f, nlb, blk, partial))) return rc;
  u64 tot = 0;
  RT_CHECK(rt_d2h(&tot, blk + nlb, sizeof tot, c->stream));
  const u64 nc = tot & 0xFFFFFFFFull, nd = tot >> 32;
  *n_chains = nc;
  *n_data_lines = nd;
  if (fill) {
    if ((nc && !d_heads) || (nd && !d_lines)) return fail(WGA_E_INVALID_ARG, "null array", nullptr);
    if (cap_chains < nc) return fail(WGA_E_TOO_SMALL, "d_heads too small", nullptr);
    if (cap_lines < nd) return fail(WGA_E_TOO_SMALL, "d_lines too small", nullptr);
    RT_CHECK(rt_h2d(d_line_off + nc, &nd, sizeof nd, c->stream));
  }
  RT_CHECK(rt_memset(first_bad, 0xFF, sizeof(u64), c->stream));
  WGA_LAUNCH(k_chain_parse, nlb, WGA_BLOCK, c->stream, d_text, (u64)n_bytes, L.n_lines, L.n_newlines, L.n_delims,
             (const u64*)L.delims, (const u64*)L.nl_idx, (const u64*)blk, first_bad,
             fill ? (wga_chain_head_dev*)d_heads : (wga_chain_head_dev*)nullptr, fill ? (u64*)d_lines : (u64*)nullptr,
             fill ? (u64*)d_line_off : (u64*)nullptr);
  LAUNCH_CHECK();
  u64 bad = WGA_NONE;
  RT_CHECK(rt_d2h(&bad, first_bad, sizeof bad, c->stream));
  *first_bad_line = bad;
  *status = bad == WGA_NONE ? WGA_CHAIN_OK : WGA_CHAIN_FALLBACK;
  return WGA_OK;
}

int wga_chain_line_off_rebase(wga_ctx* c, uint32_t n, const uint64_t* d_line_off, uint64_t* d_out) {
  int rc = ctx_bind(c);
  if (rc) return rc;
  if (!d_line_off || !d_out) return fail(WGA_E_INVALID_ARG, "null array", nullptr);
  if (d_line_off == d_out) return fail(WGA_E_INVALID_ARG, "d_out must not be d_line_off", nullptr);
  WGA_LAUNCH(k_chain_rebase, (u32)(((u64)n + 1u + 255u) / 256u), WGA_BLOCK, c->stream, n, (const u64*)d_line_off, (u64*)d_out);
  LAUNCH_CHECK();
  return WGA_OK;
}

int wga_fasta_pool(wga_ctx* c, const uint8_t* d_text, uint64_t n_bytes, uint64_t* n_contigs, uint64_t* pool_bytes,
                   uint8_t* d_pool, wga_fa_contig* d_contigs) {
  static_assert(sizeof(wga_fa_contig) == sizeof(wga_fa_contig_dev), "wga_fa_contig layout");
  int rc = ctx_bind(c);
  if (rc) return rc;
  if (!n_contigs || !pool_bytes) return fail(WGA_E_INVALID_ARG, "null count", nullptr);
  if (n_bytes && !d_text) return fail(WGA_E_INVALID_ARG, "d_text null", nullptr);
  if (n_bytes == 0) {
    *n_contigs = *pool_bytes = 0;
    return WGA_OK;
  }
  const u64 nb64 = (n_bytes + 4095u) / 4096u;
  if (nb64 > 0x7FFFFFFFull) return fail(WGA_E_INVALID_ARG, "text too large for one call", nullptr);
  const u32 nb = (u32)nb64;
  /* scratch: block counts | their exclusive scan (+ total) | scan partials | (count call only) the contig table */
  void* ws;
  const size_t head = ((size_t)nb * 2 + 2 + (size_t)nb / 1024 + 4) * sizeof(u64);
  if ((rc = ctx_scratch(c, head, &ws))) return rc;
  u64* blk = (u64*)ws;
  u64* blk_off = blk + nb;
  u64* partial = blk_off + nb + 1;
  ScanPlain sp;
  sp.in = blk;
  WGA_LAUNCH(k_fa_headers<false>, nb, WGA_BLOCK, c->stream, d_text, (u64)n_bytes, blk, (const u64*)nullptr,
             (wga_fa_contig_dev*)nullptr);
  LAUNCH_CHECK();
  if ((rc = run_scan_ws(c, sp, nb, blk_off, partial))) return rc;
  u64 nh = 0;
  RT_CHECK(rt_d2h(&nh, blk_off + nb, sizeof nh, c->stream));
  wga_fa_contig_dev* contigs = (wga_fa_contig_dev*)d_contigs;
  if (!d_pool) { /* the count call keeps its own contig table in the scratch arena */
    const size_t need = head + 64 + (size_t)nh * sizeof(wga_fa_contig_dev);
    if (c->scratch.cap < need) { /* regrowing frees the arena: start again with room for the table */
      if ((rc = ctx_scratch(c, need, &ws))) return rc;
      blk = (u64*)ws;
      blk_off = blk + nb;
      partial = blk_off + nb + 1;
      sp.in = blk;
      WGA_LAUNCH(k_fa_headers<false>, nb, WGA_BLOCK, c->stream, d_text, (u64)n_bytes, blk, (const u64*)nullptr,
                 (wga_fa_contig_dev*)nullptr);
      LAUNCH_CHECK();
      if ((rc = run_scan_ws(c, sp, nb, blk_off, partial))) return rc;
    }
    contigs = (wga_fa_contig_dev*)((char*)ws + ((head + 63) & ~(size_t)63));
  } else if (nh && !d_contigs) {
    return fail(WGA_E_INVALID_ARG, "d_contigs null", nullptr);
  }
  if (nh) {
    WGA_LAUNCH(k_fa_headers<true>, nb, WGA_BLOCK, c->stream, d_text, (u64)n_bytes, blk, (const u64*)blk_off, contigs);
    LAUNCH_CHECK();
    WGA_LAUNCH(k_fa_header_ends, (u32)((nh + 255) / 256), WGA_BLOCK, c->stream, d_text, (u64)n_bytes, nh, contigs);
    LAUNCH_CHECK();
  }
  WGA_LAUNCH(k_fa_bases<false>, nb, WGA_BLOCK, c->stream, d_text, (u64)n_bytes, nh, contigs, blk, (const u64*)nullptr,
             (u8*)nullptr);
  LAUNCH_CHECK();
  if ((rc = run_scan_ws(c, sp, nb, blk_off, partial))) return rc;
  u64 total = 0;
  RT_CHECK(rt_d2h(&total, blk_off + nb, sizeof total, c->stream));
  *n_contigs = nh;
  *pool_bytes = total;
  if (!d_pool) return WGA_OK;
  WGA_LAUNCH(k_fa_bases<true>, nb, WGA_BLOCK, c->stream, d_text, (u64)n_bytes, nh, contigs, blk, (const u64*)blk_off, d_pool);
  LAUNCH_CHECK();
  if (nh) {
    WGA_LAUNCH(k_fa_finish, (u32)((nh + 255) / 256), WGA_BLOCK, c->stream, (u64)n_bytes, nh, total, contigs);
    LAUNCH_CHECK();
    WGA_LAUNCH(k_fa_lengths, (u32)((nh + 255) / 256), WGA_BLOCK, c->stream, nh, total, contigs);
    LAUNCH_CHECK();
  }
  return WGA_OK;
}

/* K18: bytes in HBM -> BGZF members (wga_k18_bgzf_deflate.h) */
static const uint8_t k_bgzf_eof[28] = {0x1f, 0x8b, 0x08, 0x04, 0, 0, 0, 0, 0, 0xff, 0x06, 0, 0x42, 0x43,
                                       0x02, 0, 0x1b, 0, 0x03, 0, 0, 0, 0, 0, 0, 0, 0, 0};
uint64_t wga_bgzf_bound(uint64_t n_bytes) {
  const uint64_t members = (n_bytes + WGA_BGZF_IN - 1u) / WGA_BGZF_IN;
  return n_bytes + members * (uint64_t)(WGA_BGZF_HDR + 5u + WGA_BGZF_TRAILER) + sizeof k_bgzf_eof;
}
int wga_bgzf_compress(wga_ctx* c, const uint8_t* d_in, uint64_t n_bytes, uint8_t* d_out, uint64_t out_cap,
                      uint64_t* out_bytes, int eof_marker) {
  int rc = ctx_bind(c);
  if (rc) return rc;
  if (!out_bytes) return fail(WGA_E_INVALID_ARG, "out_bytes null", nullptr);
  if (n_bytes && !d_in) return fail(WGA_E_INVALID_ARG, "d_in null", nullptr);
  const u64 nb64 = (n_bytes + WGA_BGZF_IN - 1u) / WGA_BGZF_IN;
  if (nb64 > 0x7FFFFFFFull) return fail(WGA_E_INVALID_ARG, "more than 2^31 members in one call", nullptr);
  const u32 nb = (u32)nb64;
  const u64 tail = eof_marker ? sizeof k_bgzf_eof : 0u;
  u64 total = 0;
  if (nb) {
    /* scratch: member sizes | their exclusive scan (+ total) | scan partials | crc + kind per member | code lengths */
    void* ws;
    const size_t words = (size_t)nb * 2 + 2 + (size_t)nb / 1024 + 4;
    const size_t head = words * sizeof(u64);
    const size_t need = head + (size_t)nb * sizeof(wga_bgzf_member) + (size_t)nb * WGA_BGZF_LENS;
    if ((rc = ctx_scratch(c, need, &ws))) return rc;
    u64* sizes = (u64*)ws;
    u64* offs = sizes + nb;
    u64* partial = offs + nb + 1;
    wga_bgzf_member* members = (wga_bgzf_member*)((char*)ws + head);
    u8* lens = (u8*)(members + nb);
    WGA_LAUNCH(k_bgzf_plan, nb, WGA_BLOCK, c->stream, d_in, (u64)n_bytes, sizes, members, lens);
    LAUNCH_CHECK();
    ScanPlain sp;
    sp.in = sizes;
    if ((rc = run_scan_ws(c, sp, nb, offs, partial))) return rc;
    RT_CHECK(rt_d2h(&total, offs + nb, sizeof total, c->stream));
    *out_bytes = total + tail;
    if (!d_out) return WGA_OK; /* the count call */
    if (total + tail > out_cap) return fail(WGA_E_INVALID_ARG, "output buffer smaller than the compressed stream (wga_bgzf_bound)", nullptr);
    WGA_LAUNCH(k_bgzf_emit, nb, WGA_BLOCK, c->stream, d_in, (u64)n_bytes, (const u64*)offs, (const wga_bgzf_member*)members,
               (const u8*)lens, d_out);
    LAUNCH_CHECK();
  }
  *out_bytes = total + tail;
  if (tail && d_out) {
    if (total + tail > out_cap) return fail(WGA_E_INVALID_ARG, "output buffer smaller than the compressed stream (wga_bgzf_bound)", nullptr);
    RT_CHECK(rt_h2d(d_out + total, k_bgzf_eof, sizeof k_bgzf_eof, c->stream));
  }
  return WGA_OK;
}

int wga_bgzf_inflate(wga_ctx* c, const uint8_t* d_in, uint64_t in_bytes, uint32_t n_blocks, const wga_bgzf_block* d_blocks,
                     uint8_t* d_out, uint32_t* d_status) {
  int rc = ctx_bind(c);
  if (rc) return rc;
  if (n_blocks == 0) return WGA_OK;
  static_assert(sizeof(wga_bgzf_block) == sizeof(wga_bgzf_block_dev) && sizeof(wga_bgzf_block) == 24, "wga_bgzf_block layout");
  if (!d_in || !d_blocks || !d_out || !d_status) return fail(WGA_E_INVALID_ARG, "null array", nullptr);
  WGA_LAUNCH(k_bgzf_inflate, (n_blocks + 3u) / 4u, WGA_BLOCK, c->stream, d_in, (u64)in_bytes, n_blocks,
             (const wga_bgzf_block_dev*)d_blocks, d_out, (u32*)d_status);
  LAUNCH_CHECK();
  return WGA_OK;
}

int wga_bgzf_crc32(wga_ctx* c, const uint8_t* d_text, uint32_t n_blocks, const wga_bgzf_block* d_blocks, uint32_t* d_crc) {
  int rc = ctx_bind(c);
  if (rc) return rc;
  if (n_blocks == 0) return WGA_OK;
  if (!d_text || !d_blocks || !d_crc) return fail(WGA_E_INVALID_ARG, "null array", nullptr);
  WGA_LAUNCH(k_bgzf_crc32, (n_blocks + 3u) / 4u, WGA_BLOCK, c->stream, d_text, n_blocks, (const wga_bgzf_block_dev*)d_blocks,
             (u32*)d_crc);
  LAUNCH_CHECK();
  return WGA_OK;
}

int wga_pafcov_format(wga_ctx* c, const uint8_t* d_name, uint32_t name_len, const int32_t* d_cov,
                      uint64_t p0, uint32_t count, uint64_t* d_line_off, uint8_t* d_out) {
  int rc = ctx_bind(c);
  if (rc) return rc;
  if (!d_line_off || (count && !d_cov) || (name_len && !d_name)) return fail(WGA_E_INVALID_ARG, "null array", nullptr);
  ScanCovLine f;
  f.cov = (const int*)d_cov;
  f.p0 = p0;
  f.name_len = name_len;
  if (!d_out) return run_scan(c, f, count, (u64*)d_line_off);
  if (count == 0) return WGA_OK;
  WGA_LAUNCH(k_pafcov_format, (count + WGA_BED_LINES - 1u) / WGA_BED_LINES, WGA_BLOCK, c->stream, f, count, d_name,
             (const u64*)d_line_off, d_out);
  LAUNCH_CHECK();
  return WGA_OK;
}

} /* extern "C" */
