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

/* blocks recs[0 .. n) on device d (device g of the run), window by window; sink(dev, text, bytes) takes every window's text in
 * order.  Returns the first bad block's index among recs, ~0u when there is none (the windows behind it are not made). */
static uint32_t rewrite_blocks(Dev& d, int g, MafRewrite& rw, const MafInput& in, bool in_place, const MafRecord* const* recs,
                               uint32_t n, size_t budget, const std::function<void(Dev&, const uint8_t*, size_t)>& sink) {
  d.init();
  const wga_maf_rewrite_params par = rw.params(d, g);
  std::vector<wga_maf_slice_row> rows;
  std::vector<uint64_t> row0(n), bound(n);
  std::string blob;
  for (uint32_t b = 0; b < n; b++) {
    const MafRecord& r = *recs[b];
    row0[b] = rows.size();
    uint64_t rb = 13;
    for (size_t i = 0; i < r.slines.size(); i++) {
      const MafSLine& s = r.slines[i];
      wga_maf_slice_row x;
      if (in_place) {
        x.seq_off = s.seq_off;
        x.name_off = s.name_off;
      } else { /* the rows gathered from the host copy of the text (the host reader, or a device other than the reader's) */
        x.name_off = blob.size();
        blob += s.name;
        x.seq_off = blob.size();
        blob.append(s.seq_data(), s.seq_size());
      }
      x.seq_len = s.seq_size();
      x.start = s.start;
      x.size = s.align_size;
      x.src_size = s.size;
      x.name_len = (uint32_t)s.name.size();
      x.strand_neg = s.neg ? 1u : 0u;
      rows.push_back(x);
      rb += s.name.size() + (i < rw.prefixes.size() ? rw.prefixes[i].size() : 0) + 70u + s.seq_size();
    }
    bound[b] = rb;
  }
  const uint8_t* d_text = in_place ? in.d_text : nullptr;
  if (!in_place) {
    blob.append(16, '\0');
    d_text = d.upload((const uint8_t*)blob.data(), blob.size());
  }
  auto* d_rows = d.upload(rows);
  g_timer.mark("host rows + upload");
  const uint64_t max_lines = (uint64_t)1 << 31;
  for (uint32_t b0 = 0; b0 < n;) {
    std::vector<wga_maf_rewrite_block> win;
    uint64_t used = 0, lines = 0;
    uint32_t b1 = b0;
    for (; b1 < n; b1++) {
      const uint64_t nr = recs[b1]->slines.size();
      if (b1 > b0 && (used + bound[b1] > budget || lines + nr > max_lines)) break;
      win.push_back(wga_maf_rewrite_block{row0[b1], (uint32_t)nr, 0});
      used += bound[b1];
      lines += nr;
    }
    auto* d_blocks = d.upload(win);
    void* d_work = d.alloc((size_t)wga_maf_rewrite_work_bytes((uint32_t)win.size(), lines));
    uint64_t bytes = 0;
    uint32_t kept = 0, bad = 0xFFFFFFFFu;
    d.check(wga_maf_rewrite(d.ctx, d_text, d_rows, (uint32_t)win.size(), d_blocks, lines, &par, d_work, &bytes, &kept, &bad, nullptr));
    auto* d_out = (uint8_t*)d.alloc((size_t)bytes + 16);
    d.check(wga_maf_rewrite(d.ctx, d_text, d_rows, (uint32_t)win.size(), d_blocks, lines, &par, d_work, &bytes, &kept, &bad, d_out));
    d.release(d_work);
    d.release(d_blocks);
    sink(d, d_out, (size_t)bytes); /* the sink releases d_out or keeps it */
    if (bad != 0xFFFFFFFFu) return b0 + bad;
    b0 = b1;
  }
  return 0xFFFFFFFFu;
}

/* the driver of both commands: pieces, windows and --gpus N as cmd_chunk (each device a contiguous range of a piece's blocks,
 * device 0 streams first and the others hold their text in HBM; the bytes are those of one device) */
static int rewrite_maf(const std::string* input, const std::string& header, MafRewrite& rw, Output& out) {
  Dev d;
  MafDevices md(d);
  rw.on_dev.resize((size_t)md.count());
  size_t budget = (size_t)1 << 28;
  if (const char* e = getenv("WGA_MAF_REWRITE_OUT_BYTES")) budget = std::max<size_t>(1, (size_t)strtoull(e, nullptr, 10));
  std::string pending_error;
  MafChunks chunks(input);
  chunks.keep_going = true;
  out.write(header + "\n"); /* the input's header is dropped */
  MafInput min;
  g_timer.mark("host");
  for (;;) {
    bool more = false;
    try {
      more = chunks.next(d, min);
    } catch (Error& e) {
      pending_error = e.msg;
    }
    g_timer.mark("read + upload + split");
    if (!more) break;
    const std::vector<const MafRecord*> all = all_records(min.recs);
    const uint32_t n = (uint32_t)all.size();
    const int ng = md.count();
    bool bad = false;
    if (ng == 1) {
      bad = rewrite_blocks(d, 0, rw, min, min.on_device, all.data(), n, budget, [&](Dev& dg, const uint8_t* t, size_t bytes) {
              stream_out(dg, out, t, bytes);
              dg.release((void*)t);
            }) != 0xFFFFFFFFu;
    } else {
      std::vector<std::vector<std::pair<const uint8_t*, size_t>>> texts((size_t)ng);
      std::vector<uint32_t> first_bad((size_t)ng, 0xFFFFFFFFu);
      on_devices(ng, [&](int g) {
        const uint32_t lo = (uint32_t)((uint64_t)n * g / ng), hi = (uint32_t)((uint64_t)n * (g + 1) / ng);
        if (lo == hi) return;
        first_bad[(size_t)g] = rewrite_blocks(md.dev(g), g, rw, min, g == 0 && min.on_device, all.data() + lo, hi - lo, budget,
                                              [&](Dev& dg, const uint8_t* t, size_t bytes) {
                                                if (g == 0) {
                                                  stream_out(dg, out, t, bytes, false);
                                                  dg.release((void*)t);
                                                } else {
                                                  texts[(size_t)g].emplace_back(t, bytes);
                                                }
                                              });
      });
      for (int g = 0; g < ng && !bad; g++) { /* the text ends behind the first device that met a bad block */
        for (const auto& t : texts[(size_t)g]) stream_out(md.dev(g), out, t.first, t.second);
        bad = first_bad[(size_t)g] != 0xFFFFFFFFu;
      }
    }
    md.release_all();
    if (bad) pending_error = rw.bad_message;
    if (pending_error.empty() && !min.error.empty()) pending_error = min.error;
    if (!pending_error.empty()) break;
  }
  out.close();
  g_timer.mark("write");
  if (!pending_error.empty()) fail(pending_error);
  return leave(0);
}

/* ---- filter (tools/filter.rs, utils.rs:540-576) --------------------------------------------------------------------------------
 * MAF: K22 with the thresholds (`-a` is ignored, as in the reference).  PAF and chain are host paths: the records are
 * re-serialised field by field (csv writer / the chain Display impls), which no kernel of this engine does. */
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
  std::string err, text;
  const std::vector<ChainRecord> recs = parse_chain(read_all(input), &err);
  for (const ChainRecord& r : recs) {
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
    for (size_t k = 0; k + 2 < r.lines.size(); k += 3) { /* chain.rs:92-100 */
      text.push_back('\n');
      append_u64(text, r.lines[k]);
      text.push_back('\t');
      append_u64(text, r.lines[k + 1]);
      text.push_back('\t');
      append_u64(text, r.lines[k + 2]);
    }
    text += "\n\n";
  }
  out.write(text);
  out.close();
  if (!err.empty()) fail(err); /* the chains in front of a reader error are written first */
  return leave(0);
}
