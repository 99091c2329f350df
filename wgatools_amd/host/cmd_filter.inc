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
 * MAF: K22 with the thresholds (`-a` is ignored, as in the reference).  PAF: K24 selects and copies the lines of every piece whose
 * bytes the csv writer would reproduce, and groups the name pairs of `-a`; the other pieces are re-serialised field by field on
 * the host (csv writer).  Chain: a plain file is read on the device (ChainInput, K23) and written there (K25, wga_chain_filter:
 * for a file the splitter takes the score's f64 Display is its plain decimal, the names are spans of the text, everything else
 * is a u64); the kept text comes back once.  A file the splitter leaves to the host reader is formatted on the host as before. */
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

/* ---- filter -f paf on the device (K24) -----------------------------------------------------------------------------------------
 * For a plain line whose nine numbers are in canonical decimal the csv writer reproduces the line's bytes, so a piece whose lines
 * are all of that kind (wga_paf_filter's exactness check: no fallback line of the splitter, no byte >= 0x80, no `+5` / `007`) is
 * filtered where it was uploaded: the line table stays on the device, no record is built, and the kept lines leave through the
 * pinned-buffer sink of the MAF window commands.  Any other piece goes through parse_paf + filter_paf_row with the same record,
 * line and byte counters, so device and host pieces may alternate within one file and the reader's error text is what it was.
 * WGA_PAF_READER=host sends every piece to the host path.  The PAF filter runs on device 0 whatever --gpus says. */
struct PafOnDev {
  size_t owned0 = 0; /* the Dev's buffers in front of this piece's */
  uint8_t* d_text = nullptr;
  wga_paf_line* d_lines = nullptr;
  void* d_work = nullptr;
  uint64_t n_bytes = 0, n_lines = 0, n_ok = 0; /* n_ok: the piece's records */
  uint64_t bytes = 0, kept = 0;                /* of the last count call */
};
static bool paf_filter_host_forced() { return env_is("WGA_PAF_READER", "host"); }
/* the piece on the device, split, and through the count call at thresholds 0 (every record kept: n_ok).  False, with nothing left
 * on the device: the piece is the host path's. */
static bool paf_filter_upload(Dev& d, std::string& text, PafOnDev& p) {
  if (paf_filter_host_forced() || text.empty() || text.size() >= 0xFFFFFFF0ull) return false;
  d.init();
  p = PafOnDev();
  p.owned0 = d.owned.size();
  p.n_bytes = text.size();
  text.append(16, '\0'); /* slack behind the text for whole-vector loads */
  p.d_text = d.upload((const uint8_t*)text.data(), text.size());
  text.resize(text.size() - 16);
  g_timer.mark("upload");
  d.check(wga_paf_split(d.ctx, p.d_text, p.n_bytes, &p.n_lines, nullptr, 0));
  p.d_lines = (wga_paf_line*)d.alloc((size_t)(p.n_lines + 1) * sizeof(wga_paf_line));
  d.check(wga_paf_split(d.ctx, p.d_text, p.n_bytes, &p.n_lines, p.d_lines, p.n_lines));
  p.d_work = d.alloc((size_t)wga_paf_filter_work_bytes(p.n_lines));
  const wga_paf_filter_params all = {0, 0, nullptr, nullptr};
  uint64_t inexact = WGA_NONE;
  d.check(wga_paf_filter(d.ctx, p.d_text, p.n_bytes, p.d_lines, p.n_lines, &all, p.d_work, &p.bytes, &p.kept, &inexact, nullptr));
  p.n_ok = p.kept;
  g_timer.mark("device split + exactness");
  if (inexact == WGA_NONE) return true;
  d.release_to(p.owned0);
  return false;
}
/* the text of the piece's kept lines: the count call (unless `counted`: the one at thresholds 0 is the caller's), the fill, out */
static void paf_filter_write(Dev& d, PafOnDev& p, const wga_paf_filter_params& par, bool counted, Output& out) {
  uint64_t inexact = WGA_NONE;
  if (!counted)
    d.check(wga_paf_filter(d.ctx, p.d_text, p.n_bytes, p.d_lines, p.n_lines, &par, p.d_work, &p.bytes, &p.kept, &inexact, nullptr));
  if (p.bytes == 0) return;
  auto* d_out = (uint8_t*)d.alloc((size_t)p.bytes + 16);
  d.check(wga_paf_filter(d.ctx, p.d_text, p.n_bytes, p.d_lines, p.n_lines, &par, p.d_work, &p.bytes, &p.kept, &inexact, d_out));
  stream_out(d, out, d_out, (size_t)p.bytes);
}

int paf_filter_paths(const std::string* input) { /* `__paf_filter_path`: one line per piece */
  Dev d;
  PafChunks chunks(input, true);
  std::string piece;
  uint64_t line0 = 0, byte0 = 0;
  while (chunks.next_text(piece, line0, byte0)) {
    PafOnDev p;
    const bool dev = paf_filter_upload(d, piece, p);
    if (dev) d.release_to(p.owned0);
    printf("%s\n", dev ? "device" : "host");
  }
  return 0;
}

int cmd_filter_paf(const std::string* input, uint64_t min_block, uint64_t min_query, const uint64_t* min_align, Output& out) {
  Dev d; /* started by the first piece that takes the device path */
  PafChunks chunks(input, true);
  std::string pending_error, text;
  uint64_t recs_before = 0, line0 = 0, byte0 = 0;
  auto next = [&]() {
    try {
      return chunks.next_text(text, line0, byte0);
    } catch (Error& e) { /* the records in front of a reader error are written first */
      pending_error = e.msg;
      return false;
    }
  };
  auto host_records = [&](const std::string& piece, uint64_t l0, uint64_t b0, std::vector<PafRecord>& recs) {
    try {
      recs = parse_paf(piece, recs_before, l0, b0);
      return true;
    } catch (Error& e) {
      pending_error = e.msg;
      return false;
    }
  };
  g_timer.mark("host");
  if (min_align) { /* filter.rs:108-160: the whole input, the pairs' sums, then the records in input order */
    log_warn("`min_align_size` is set, will not filter paf `min_block_size` and `min_query_size`");
    typedef std::map<std::pair<std::string, std::string>, uint64_t> Sums;
    Sums sum;
    struct Piece {
      std::string text;
      bool on_dev = false;
      std::vector<uint64_t*> pair_sum; /* device piece: the global sum of every pair of the piece, in the device's numbering */
      std::vector<PafRecord> recs;     /* host piece */
    };
    std::vector<Piece> pieces;
    PafOnDev resident; /* the latest device piece stays where it is: with one piece in all, the second pass needs no upload */
    uint32_t* d_resident_pol = nullptr;
    bool have_resident = false;
    /* wga_paf_pairs on a piece that is on the device: d_pol, and the piece's pairs if asked for */
    auto device_pairs = [&](PafOnDev& p, uint32_t** d_pol, std::vector<wga_paf_pair>* pairs) {
      void* d_work = d.alloc((size_t)wga_paf_pairs_work_bytes(p.n_lines));
      uint64_t np = 0;
      d.check(wga_paf_pairs(d.ctx, p.d_text, p.n_bytes, p.d_lines, p.n_lines, d_work, &np, nullptr, nullptr, 0));
      *d_pol = (uint32_t*)d.alloc((size_t)(p.n_lines + 1) * sizeof(uint32_t));
      auto* d_pairs = (wga_paf_pair*)d.alloc((size_t)(np + 1) * sizeof(wga_paf_pair));
      d.check(wga_paf_pairs(d.ctx, p.d_text, p.n_bytes, p.d_lines, p.n_lines, d_work, &np, *d_pol, d_pairs, np));
      if (pairs) {
        pairs->resize((size_t)np);
        if (np) d.download(pairs->data(), d_pairs, (size_t)np);
      }
      d.release(d_pairs);
      d.release(d_work);
      return np;
    };
    while (next()) {
      if (have_resident) d.release_to(resident.owned0);
      have_resident = false;
      Piece pc;
      PafOnDev p;
      if (paf_filter_upload(d, text, p)) {
        pc.on_dev = true;
        std::vector<wga_paf_pair> pairs;
        device_pairs(p, &d_resident_pol, &pairs);
        for (const wga_paf_pair& q : pairs) { /* the names come from the host copy of the text */
          uint64_t& g = sum[{std::string(text, (size_t)q.qname_off, q.qname_len), std::string(text, (size_t)q.tname_off, q.tname_len)}];
          g += q.sum; /* wraps, as the release build does */
          pc.pair_sum.push_back(&g);
        }
        recs_before += p.n_ok;
        resident = p;
        have_resident = true;
        g_timer.mark("device pairs + host merge");
      } else {
        if (!host_records(text, line0, byte0, pc.recs)) break;
        for (const PafRecord& r : pc.recs) sum[{r.query_name, r.target_name}] += r.target_end - r.target_start;
        recs_before += pc.recs.size();
      }
      if (pc.on_dev) { /* a device piece is uploaded again for the second pass; a host piece has its records */
        pc.text = std::move(text);
        text = std::string();
      }
      pieces.push_back(std::move(pc));
    }
    if (pending_error.empty()) { /* the reference collects before it writes: an error leaves no record */
      for (size_t k = 0; k < pieces.size(); k++) {
        Piece& pc = pieces[k];
        if (!pc.on_dev) {
          std::string rows;
          for (const PafRecord& r : pc.recs)
            if (sum[{r.query_name, r.target_name}] >= *min_align) filter_paf_row(rows, r);
          out.write(rows);
          continue;
        }
        PafOnDev p = resident;
        uint32_t* d_pol = d_resident_pol;
        if (!(have_resident && pieces.size() == 1)) {
          if (have_resident) d.release_to(resident.owned0);
          have_resident = false;
          if (!paf_filter_upload(d, pc.text, p)) fail("internal error: a PAF piece changed between the passes");
          if (device_pairs(p, &d_pol, nullptr) != pc.pair_sum.size()) fail("internal error: a PAF piece's pairs changed between the passes");
        }
        std::vector<uint8_t> keep(pc.pair_sum.size() + 16, 0);
        for (size_t j = 0; j < pc.pair_sum.size(); j++) keep[j] = *pc.pair_sum[j] >= *min_align ? 1 : 0;
        const wga_paf_filter_params par = {0, 0, d_pol, d.upload(keep)};
        paf_filter_write(d, p, par, false, out);
        d.release_to(p.owned0);
        have_resident = false;
      }
    }
  } else {
    const wga_paf_filter_params par = {min_block, min_query, nullptr, nullptr};
    while (next()) {
      PafOnDev p;
      if (paf_filter_upload(d, text, p)) {
        paf_filter_write(d, p, par, min_block == 0 && min_query == 0, out);
        d.release_to(p.owned0);
        recs_before += p.n_ok;
        continue;
      }
      std::vector<PafRecord> recs;
      if (!host_records(text, line0, byte0, recs)) break;
      std::string rows;
      for (const PafRecord& r : recs)
        if (!(r.target_end - r.target_start < min_block || r.query_length < min_query)) filter_paf_row(rows, r);
      out.write(rows);
      recs_before += recs.size();
    }
  }
  out.close();
  g_timer.mark("write");
  if (!pending_error.empty()) fail(pending_error);
  return leave(0);
}

/* ---- filter -f chain on the device (K25) ---------------------------------------------------------------------------------------
 * A file the chain splitter takes stays in HBM whole (text, heads, data lines, offsets); wga_chain_filter selects the chains and
 * writes their text there, and the kept bytes leave through the pinned-buffer sink (`.gz`: deflated on the device first).  Any
 * other input (WGA_CHAIN_READER=host, a fallback file, an empty file, 4 GiB or more) is formatted on the host from the host
 * reader's records, the chains in front of a reader error first.  Runs on device 0 whatever --gpus says. */
int chain_filter_path(const std::string* input) { /* `__chain_filter_path` */
  Dev d;
  ChainInput in = load_chain(d, input, true);
  printf("%s\n", in.on_device ? "device" : "host");
  return 0;
}

static int filter_chain_device(Dev& d, const ChainInput& in, uint64_t min_block, uint64_t min_query, Output& out) {
  const wga_chain_filter_params par = {min_block, min_query};
  uint64_t kept = 0;
  const DevText t = two_call_text(
      d, (size_t)wga_chain_filter_work_bytes(in.n_chains, in.n_data_lines) + 16, [&](void* d_work, uint64_t* bytes, uint8_t* d_out) {
        return wga_chain_filter(d.ctx, in.d_text, in.n_bytes, in.d_heads, in.n_chains, in.d_lines, in.d_line_off, &par, d_work, bytes, &kept,
                                d_out);
      });
  if (t.bytes) {
    d.check(wga_sync(d.ctx));
    g_timer.mark("device text");
    stream_out(d, out, t.d_out, t.bytes, false);
    g_timer.mark("copy out + write");
  }
  out.close();
  return leave(0);
}

int cmd_filter_chain(const std::string* input, uint64_t min_block, uint64_t min_query, Output& out) {
  std::string text;
  Dev d;
  ChainInput in = load_chain(d, input, true);
  if (in.on_device) return filter_chain_device(d, in, min_block, min_query, out);
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
