/* cmd_filter.inc — part of wgatools_main.cpp (included there, inside its namespace: the commands share the device helpers, readers and
 * writers defined in front of the include). */
/* ---- the MAF block rewriter of filter and rename (K22, wga_maf_rewrite) --------------------------------------------------------
 * Both commands write a new copy of every surviving block through the reference's record writer (maf.rs:566-581).  The blocks
 * come from the piece reader (MafChunks: device splitter or host reader); a piece's rows go into one row table and its blocks
 * through K22 in WINDOWS of consecutive blocks whose text is bounded by WGA_MAF_REWRITE_OUT_BYTES (256 MiB; a block above the
 * bound is a window of its own).  Which blocks survive is decided on the device from the row table: the host never compares a
 * field.  A BAD block (filter: fewer than two rows; rename: a row count that differs from the prefixes') ends the output in
 * front of it. */
struct MafRewrite {
  bool filter = false;
  uint64_t min_block = 0, min_query = 0;
  std::vector<std::string> prefixes;
  std::string bad_message;
  /* the prefixes on every device: uploaded once, by the device's own worker, and kept for the run (not among Dev::owned, which
   * is released piece by piece) */
  struct OnDev {
    uint8_t* text = nullptr;
    uint32_t* off = nullptr;
  };
  std::vector<OnDev> on_dev;
  wga_maf_rewrite_params params(Dev& d, int g) {
    wga_maf_rewrite_params p;
    p.min_block_size = min_block;
    p.min_query_size = min_query;
    p.filter = filter ? 1u : 0u;
    p.n_prefix = (uint32_t)prefixes.size();
    p.d_prefix_text = nullptr;
    p.d_prefix_off = nullptr;
    if (!prefixes.empty()) {
      OnDev& o = on_dev[(size_t)g];
      if (!o.off) {
        std::string blob;
        std::vector<uint32_t> off{0};
        for (const std::string& s : prefixes) {
          blob += s;
          off.push_back((uint32_t)blob.size());
        }
        blob.append(16, '\0');
        void *t = nullptr, *f = nullptr;
        d.check(wga_malloc(d.ctx, blob.size(), &t));
        d.check(wga_malloc(d.ctx, off.size() * 4, &f));
        d.check(wga_memcpy_h2d(d.ctx, t, blob.data(), blob.size()));
        d.check(wga_memcpy_h2d(d.ctx, f, off.data(), off.size() * 4));
        o.text = (uint8_t*)t;
        o.off = (uint32_t*)f;
      }
      p.d_prefix_text = o.text;
      p.d_prefix_off = o.off;
    }
    return p;
  }
};

/* blocks recs[0 .. n) on device d (device g of the run), window by window.  Returns whether a window met a bad block (the
 * windows behind it are not made). */
static bool rewrite_blocks(Dev& d, int g, MafRewrite& rw, const MafInput& in, bool in_place, const MafRecord* const* recs,
                           uint32_t n, size_t budget, const MafSink& sink) {
  d.init();
  const wga_maf_rewrite_params par = rw.params(d, g);
  const MafRowTable<wga_maf_slice_row> t = maf_row_table<wga_maf_slice_row>(d, in, in_place, recs, n);
  std::vector<uint64_t> bound(n); /* of a block's text: prefix, name, three 20-digit numbers and the row per line */
  for (uint32_t b = 0; b < n; b++) {
    const std::vector<MafSLine>& sl = recs[b]->slines;
    bound[b] = 13;
    for (size_t i = 0; i < sl.size(); i++)
      bound[b] += sl[i].name.size() + (i < rw.prefixes.size() ? rw.prefixes[i].size() : 0) + 70u + sl[i].seq_size();
  }
  g_timer.mark("host rows + upload");
  const uint64_t max_lines = (uint64_t)1 << 31;
  for (uint32_t b0 = 0; b0 < n;) {
    std::vector<wga_maf_rewrite_block> win;
    uint64_t used = 0, lines = 0;
    uint32_t b1 = b0;
    for (; b1 < n; b1++) {
      const uint64_t nr = recs[b1]->slines.size();
      if (b1 > b0 && (used + bound[b1] > budget || lines + nr > max_lines)) break;
      win.push_back(wga_maf_rewrite_block{t.row0[b1], (uint32_t)nr, 0});
      used += bound[b1];
      lines += nr;
    }
    auto* d_blocks = d.upload(win);
    const uint32_t nb = (uint32_t)win.size();
    uint32_t kept = 0, bad = 0xFFFFFFFFu;
    maf_window_call(d, (size_t)wga_maf_rewrite_work_bytes(nb, lines), d_blocks, [&](void* d_work, uint64_t* bytes, uint8_t* d_out) {
      return wga_maf_rewrite(d.ctx, t.d_text, t.d_rows, nb, d_blocks, lines, &par, d_work, bytes, &kept, &bad, d_out);
    }, sink);
    if (bad != 0xFFFFFFFFu) return true;
    b0 = b1;
  }
  return false;
}

/* the driver of both commands: pieces, windows and --gpus N are maf_pieces' */
static int rewrite_maf(const std::string* input, const std::string& header, MafRewrite& rw, Output& out) {
  rw.on_dev.resize((size_t)std::max(1, g_gpus)); /* one slot per device of the run */
  return maf_pieces(
      input, header, "WGA_MAF_REWRITE_OUT_BYTES", out,
      [&](const MafPiece& p, int g, Dev& dg, bool in_place, uint32_t lo, uint32_t hi, const MafSink& sink) {
        return rewrite_blocks(dg, g, rw, p.in, in_place, p.recs.data() + lo, hi - lo, p.budget, sink);
      },
      rw.bad_message);
}

/* ---- filter (tools/filter.rs, utils.rs:540-576) --------------------------------------------------------------------------------
 * MAF: K22 with the thresholds (`-a` is ignored, as in the reference).  PAF and chain are written on the host: the records are
 * re-serialised field by field (csv writer / the chain Display impls), which no kernel of this engine does; a plain chain file
 * is read on the device (ChainInput) and its data lines come back in one copy. */
static const char* kFilterNoQuery = "panic: a block with a single s-line has no query row (maf.rs:430 index out of bounds)";

int cmd_filter_maf(const std::string* input, uint64_t min_block, uint64_t min_query, Output& out) {
  MafRewrite rw;
  rw.filter = true;
  rw.min_block = min_block;
  rw.min_query = min_query;
  rw.bad_message = kFilterNoQuery;
  return rewrite_maf(input, "#maf version=1.6 filter=blocksize>=" + std::to_string(min_block) + " querysize>=" + std::to_string(min_query),
                     rw, out);
}

static void filter_paf_row(std::string& rows, const PafRecord& r) { /* csv writer: tab, flexible, no header; paf.rs:50-65 */
  append_csv_field(rows, r.query_name, '\t');
  const uint64_t a[] = {r.query_length, r.query_start, r.query_end};
  for (uint64_t v : a) {
    rows.push_back('\t');
    append_u64(rows, v);
  }
  rows += r.neg ? "\t-\t" : "\t+\t";
  append_csv_field(rows, r.target_name, '\t');
  const uint64_t b2[] = {r.target_length, r.target_start, r.target_end, r.matches, r.block_length, r.mapq};
  for (uint64_t v : b2) {
    rows.push_back('\t');
    append_u64(rows, v);
  }
  for (const std::string& tg : r.tags) {
    rows.push_back('\t');
    append_csv_field(rows, tg, '\t');
  }
  rows.push_back('\n');
}

int cmd_filter_paf(const std::string* input, uint64_t min_block, uint64_t min_query, const uint64_t* min_align, Output& out) {
  Dev d; /* never started: with tags wanted every piece goes through the host reader */
  PafChunks chunks(input, true);
  PafInput pin;
  std::string pending_error;
  auto next = [&]() {
    try {
      return chunks.next(d, pin);
    } catch (Error& e) { /* the records in front of a reader error are written first */
      pending_error = e.msg;
      return false;
    }
  };
  if (min_align) { /* filter.rs:108-160: the whole input, the pairs' sums, then the records in input order */
    log_warn("`min_align_size` is set, will not filter paf `min_block_size` and `min_query_size`");
    std::vector<PafRecord> all;
    std::map<std::pair<std::string, std::string>, uint64_t> sum;
    while (next())
      for (PafRecord& r : pin.recs) {
        sum[{r.query_name, r.target_name}] += r.target_end - r.target_start; /* wraps, as the release build does */
        all.push_back(std::move(r));
      }
    if (pending_error.empty()) { /* the reference collects before it writes: an error leaves no record */
      std::string rows;
      for (const PafRecord& r : all)
        if (sum[{r.query_name, r.target_name}] >= *min_align) filter_paf_row(rows, r);
      out.write(rows);
    }
  } else {
    while (next()) {
      std::string rows;
      for (const PafRecord& r : pin.recs)
        if (!(r.target_end - r.target_start < min_block || r.query_length < min_query)) filter_paf_row(rows, r);
      out.write(rows);
    }
  }
  out.close();
  if (!pending_error.empty()) fail(pending_error);
  return leave(0);
}

int cmd_filter_chain(const std::string* input, uint64_t min_block, uint64_t min_query, Output& out) {
  std::string text;
  Dev d;
  ChainInput in = load_chain(d, input);
  if (in.on_device) in.fetch_lines(d); /* the text is formatted here: the data lines come back once */
  const std::string& err = in.error;
  for (size_t i = 0; i < in.recs.size(); i++) {
    const ChainRecord& r = in.recs[i];
    if (r.target_end - r.target_start < min_block || r.query_size < min_query) continue;
    text += "chain\t" + format_chain_score(r.score) + "\t" + r.target_name + "\t";
    append_u64(text, r.target_size);
    text += r.target_neg ? "\t-\t" : "\t+\t";
    append_u64(text, r.target_start);
    text.push_back('\t');
    append_u64(text, r.target_end);
    text += "\t" + r.query_name + "\t";
    append_u64(text, r.query_size);
    text += r.query_neg ? "\t-\t" : "\t+\t";
    append_u64(text, r.query_start);
    text.push_back('\t');
    append_u64(text, r.query_end);
    text.push_back('\t');
    append_u64(text, r.chain_id);
    for (size_t k = 3 * (size_t)in.line_off[i]; k < 3 * (size_t)in.line_off[i + 1]; k += 3) { /* chain.rs:92-100 */
      text.push_back('\n');
      append_u64(text, in.lines[k]);
      text.push_back('\t');
      append_u64(text, in.lines[k + 1]);
      text.push_back('\t');
      append_u64(text, in.lines[k + 2]);
    }
    text += "\n\n";
  }
  out.write(text);
  out.close();
  if (!err.empty()) fail(err); /* the chains in front of a reader error are written first */
  return leave(0);
}
