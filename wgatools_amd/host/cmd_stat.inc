/* cmd_stat.inc — part of wgatools_main.cpp (included there, inside its namespace: the commands share the device helpers, readers and
 * writers defined in front of the include). */
/* ---- stat (stat.rs) ----------------------------------------------------------------------------- */
/* `wgatools --gpus N stat -f paf`: the records of a piece are counted on device fnv1a64(target_name) % N; the per-record
 * counters meet on the host, where the Pair group-by runs as on one device (stat.rs:167-223).  No collective: what a
 * reduction over devices would sum — the grand totals — is the last line of the host's merge. */
static void stat_piece_multi(std::vector<std::unique_ptr<Dev>>& devs, const PafInput& pin, std::vector<wga_cigar_counts>& counts) {
  const int ngpu = (int)devs.size();
  const size_t n = pin.recs.size();
  std::vector<std::vector<size_t>> mine(ngpu);
  for (size_t i = 0; i < n; i++) mine[fnv1a64(pin.recs[i].target_name) % (uint64_t)ngpu].push_back(i);
  std::vector<size_t> bad_at(ngpu, n);
  std::vector<std::string> bad_msg(ngpu);
  std::string text16;
  if (pin.on_device && ngpu > 1) text16 = pin.text + std::string(16, '\0');
  on_devices(ngpu, [&](int g) {
    Dev& d = *devs[g];
    d.init();
    const std::vector<size_t>& w = mine[g];
    if (w.empty()) return;
    const size_t keep = d.owned.size();
    const uint8_t* d_text = nullptr;
    if (pin.on_device) d_text = g == 0 ? pin.d_text : d.upload((const uint8_t*)text16.data(), text16.size());
    CigarTexts cigars;
    wga_cigar_batch cb;
    const std::string e = device_tokenise(d, pin, 0, (uint32_t)w.size(), cigars, &cb, nullptr, w.data(), d_text);
    const uint32_t m = cb.n; /* records before this device's first tag / tokeniser error */
    if (m) {
      auto* d_counts = (wga_cigar_counts*)d.alloc((size_t)m * sizeof(wga_cigar_counts));
      auto* d_diag = (wga_rec_diag*)d.alloc((size_t)m * sizeof(wga_rec_diag));
      d.check(wga_cigar_stat(d.ctx, &cb, d_counts, d_diag, nullptr));
      std::vector<wga_rec_diag> diag(m);
      std::vector<wga_cigar_counts> c(m);
      d.download(diag.data(), d_diag, m);
      d.download(c.data(), d_counts, m);
      for (uint32_t k = 0; k < m; k++) {
        if (diag[k].bad_op_idx != WGA_NONE) {
          bad_at[g] = w[k];
          bad_msg[g] = "CIGAR OP `" + cigar_op_token_at(cigars[k], diag[k].bad_op_idx) + "` invalid";
          break;
        }
        counts[w[k]] = c[k];
      }
    }
    if (!e.empty() && w[m] < bad_at[g]) {
      bad_at[g] = w[m];
      bad_msg[g] = e;
    }
    d.release_to(keep); /* this piece's buffers (the reader's own copy of the text on device 0 is its to release) */
  });
  size_t first_bad = n;
  for (int g = 0; g < ngpu; g++) first_bad = std::min(first_bad, bad_at[g]);
  if (first_bad < n) /* buffered driver: nothing is written on error; the first failing record in input order speaks */
    for (int g = 0; g < ngpu; g++)
      if (bad_at[g] == first_bad) fail(bad_msg[g]);
}

int cmd_stat_paf(const std::string* input, bool each, Output& out) {
  Dev d;
  PafChunks chunks(input, false);
  std::vector<StatInput> in;
  PafInput pin;
  std::vector<std::unique_ptr<Dev>> devs; /* --gpus N: devices 1 .. N - 1 next to `d` */
  while (chunks.next(d, pin)) { /* one piece of the file at a time; only the per-record statistics are kept */
    const std::vector<PafRecord>& recs = pin.recs;
    const uint32_t n = (uint32_t)recs.size();
    std::vector<wga_cigar_counts> counts(n);
    d.init();
    if (g_gpus > 1) {
      if (devs.empty()) {
        devs.emplace_back(new Dev(0));
        devs[0]->ctx = d.ctx; /* device 0's context is the reader's */
        devs[0]->own_ctx = false;
        for (int g = 1; g < g_gpus; g++) devs.emplace_back(new Dev(g));
      }
      stat_piece_multi(devs, pin, counts);
      in.reserve(in.size() + n);
      for (uint32_t k = 0; k < n; k++) {
        const PafRecord& r = recs[k];
        in.push_back(StatInput{r.target_name, r.query_name, r.target_length, r.query_length, r.target_start,
                               r.query_start, recstat_from(counts[k])});
      }
      d.release_all();
      continue;
    }
    CigarTexts cigars;
    wga_cigar_batch cb;
    const std::string e = device_tokenise(d, pin, 0, n, cigars, &cb);
    const uint32_t m = cb.n; /* records before the first tag / tokeniser error */
    if (m) {
      auto* d_counts = (wga_cigar_counts*)d.alloc((size_t)m * sizeof(wga_cigar_counts));
      auto* d_diag = (wga_rec_diag*)d.alloc((size_t)m * sizeof(wga_rec_diag));
      d.check(wga_cigar_stat(d.ctx, &cb, d_counts, d_diag, nullptr));
      std::vector<wga_rec_diag> diag(m);
      d.download(diag.data(), d_diag, m);
      d.download(counts.data(), d_counts, m);
      for (uint32_t k = 0; k < m; k++)
        if (diag[k].bad_op_idx != WGA_NONE)
          fail("CIGAR OP `" + cigar_op_token_at(cigars[k], diag[k].bad_op_idx) + "` invalid");
    }
    if (!e.empty()) fail(e); /* buffered driver: nothing is written on error */
    in.reserve(in.size() + n);
    for (uint32_t k = 0; k < n; k++) {
      const PafRecord& r = recs[k];
      in.push_back(StatInput{r.target_name, r.query_name, r.target_length, r.query_length, r.target_start,
                             r.query_start, recstat_from(counts[k])});
    }
    d.release_all();
  }
  out.write(stat_tsv(in, each));
  out.close();
  return leave(0);
}

/* A MAF input: blocks with their s-lines.  Plain files are split on the device (wga_maf_split): the rows
 * are never copied — the K3 / K4 walks read them in the uploaded file, the host keeps spans into its own
 * copy of the text for the few places that need row characters (VCF REF / ALT).  A file with a line the
 * splitter does not take goes through the host reader (the reference's errors). */
struct MafInput {
  std::shared_ptr<std::string> text = std::make_shared<std::string>();
  std::string header;
  std::vector<MafRecord> recs;
  bool on_device = false;
  uint8_t* d_text = nullptr;
  std::string error; /* keep_going: the host reader's error behind the records (they come first) */
};
MafInput maf_from_text(Dev& d, std::string&& whole_text, bool keep_going = false) {
  MafInput in;
  *in.text = std::move(whole_text);
  const std::string& text = *in.text;
  const char* force = getenv("WGA_MAF_READER"); /* "host": always the host reader (measurements) */
  if (!text.empty() && text.size() < 0xFFFFFFF0ull && !(force && strcmp(force, "host") == 0)) {
    g_timer.mark("file read");
    d.init();
    in.text->append(16, '\0'); /* slack behind the text for whole-vector loads */
    in.d_text = d.upload((const uint8_t*)text.data(), text.size());
    in.text->resize(text.size() - 16);
    g_timer.mark("upload");
    uint64_t n_lines = 0;
    d.check(wga_maf_split(d.ctx, in.d_text, text.size(), &n_lines, nullptr, 0));
    auto* d_lines = (wga_maf_line*)d.alloc((size_t)(n_lines + 1) * sizeof(wga_maf_line));
    d.check(wga_maf_split(d.ctx, in.d_text, text.size(), &n_lines, d_lines, n_lines));
    std::vector<wga_maf_line> lines((size_t)n_lines);
    if (n_lines) d.download(lines.data(), d_lines, (size_t)n_lines);
    d.release(d_lines);
    g_timer.mark("device split + line table");
    bool plain = true;
    for (const wga_maf_line& L : lines)
      if (L.status == WGA_MAF_FALLBACK) plain = false;
    if (plain) {
      in.on_device = true;
      size_t he = text.find('\n'); /* the first line is always the header (maf.rs:25-36) */
      if (he == std::string::npos) he = text.size();
      if (he > 0 && text[he - 1] == '\r') he--;
      in.header.assign(text, 0, he);
      /* a block = a maximal run of s-lines (any other line ends the block in progress); the records of a piece with millions of
       * blocks are filled by a few threads (two or more strings per block: the allocator is what this loop costs) */
      std::vector<std::pair<size_t, size_t>> runs_of_s; /* [first, behind the last) s-line of every block */
      for (size_t i = 0; i < lines.size();) {
        if (lines[i].status != WGA_MAF_SLINE) {
          i++;
          continue;
        }
        size_t j = i;
        while (j < lines.size() && lines[j].status == WGA_MAF_SLINE) j++;
        runs_of_s.emplace_back(i, j);
        i = j;
      }
      in.recs.resize(runs_of_s.size());
      auto fill = [&](size_t b0, size_t b1) {
        for (size_t b = b0; b < b1; b++) {
          MafRecord& r = in.recs[b];
          r.slines.reserve(runs_of_s[b].second - runs_of_s[b].first);
          for (size_t i = runs_of_s[b].first; i < runs_of_s[b].second; i++) {
            const wga_maf_line& L = lines[i];
            MafSLine sl;
            sl.name.assign(text, (size_t)L.name_off, L.name_len);
            sl.name_off = L.name_off;
            sl.start = L.num[0];
            sl.align_size = L.num[1];
            sl.size = L.num[2];
            sl.neg = L.strand_neg != 0;
            sl.file = text.data();
            sl.seq_off = L.seq_off;
            sl.seq_len = L.seq_len;
            r.slines.push_back(std::move(sl));
          }
        }
      };
      const size_t nb = runs_of_s.size();
      static const size_t min_blocks = getenv("WGA_MAF_FILL_MIN_BLOCKS") ? (size_t)strtoull(getenv("WGA_MAF_FILL_MIN_BLOCKS"), nullptr, 10) : 50000; /* tests: 1 */
      const unsigned T = nb >= std::max<size_t>(min_blocks, 8) ? 8u : 1u;
      if (T == 1u) {
        fill(0, nb);
      } else {
        std::vector<std::thread> th;
        for (unsigned t = 1; t < T; t++) th.emplace_back(fill, nb * t / T, nb * (t + 1) / T);
        fill(0, nb / T);
        for (auto& x : th) x.join();
      }
      g_timer.mark("host records");
      return in;
    }
    d.release(in.d_text);
    in.d_text = nullptr;
  }
  in.recs = keep_going ? parse_maf(text, &in.header, &in.error) : parse_maf(text, &in.header);
  return in;
}
MafInput load_maf(Dev& d, const std::string* input) { return maf_from_text(d, read_all(input)); }

/* A MAF input in pieces of about 1 GiB (WGA_CHUNK_BYTES) that end between blocks: a piece is cut in front of its trailing
 * run of `s` lines, which open the next piece.  The reader's rule that the file's first line is the header is kept for
 * the later pieces by a dummy first line. */
struct MafChunks {
  LineChunkReader rd;
  size_t target = (size_t)1 << 30;
  std::string pending; /* trailing s-lines of the previous piece */
  bool first = true, done = false;
  std::string header;
  std::unique_ptr<BgzfDeviceSource> bgzf; /* a bgzipped input: inflated on the device */
  bool keep_going = false; /* a piece whose host reader fails returns its records in front of the error (MafInput::error) */
  std::function<void(const std::string&)> on_piece; /* sees every piece's text, the ones without a block too (maf-index: file offsets) */
  explicit MafChunks(const std::string* input) {
    bgzf.reset(new BgzfDeviceSource());
    if (bgzf->open(input))
      rd.source = [this](char* dst, size_t want) { return bgzf->read(dst, want); };
    else
      bgzf.reset();
    rd.open(input);
    if (const char* e = getenv("WGA_CHUNK_BYTES")) target = (size_t)strtoull(e, nullptr, 10);
    if (target == 0) target = 1;
  }
  /* reader side: the text of the next piece that holds something, or false at the end of the input */
  bool produce(std::string& text) {
    while (!done) {
      text = first ? std::string() : std::string("#\n");
      const size_t skip = text.size();
      text += pending;
      pending.clear();
      const bool more = rd.next(text, target, text.size()); /* reads behind the prefix, no second copy */
      if (!more) {
        done = true;
      } else { /* cut in front of the trailing run of lines that start with 's' (the header line never counts) */
        size_t cut = text.size();
        while (cut > skip) {
          size_t ls = cut >= 2 ? text.rfind('\n', cut - 2) : std::string::npos; /* start of the last line in [.., cut) */
          ls = (ls == std::string::npos || ls + 1 < skip) ? skip : ls + 1;
          const bool is_header = first && ls == 0;
          if (text[ls] == 's' && !is_header)
            cut = ls;
          else
            break;
        }
        if (cut == skip && text.size() > skip) { /* nothing but s-lines so far: one block longer than a piece */
          pending.assign(text, skip, std::string::npos);
          continue;
        }
        pending.assign(text, cut, std::string::npos);
        text.resize(cut);
      }
      if (text.size() == skip) continue;
      first = false;
      return true;
    }
    return false;
  }
  /* the next piece is read by a helper thread while the caller works on the current one (as PafChunks does) */
  struct Ahead {
    bool ok = false;
    std::string text, err;
  } ahead;
  std::thread reader;
  bool started = false, first_seen = true;
  ~MafChunks() {
    if (reader.joinable()) reader.join();
  }
  void read_ahead() {
    reader = std::thread([this] {
      Ahead a;
      try {
        a.ok = produce(a.text);
      } catch (Error& e) {
        a.err = e.msg.empty() ? std::string("error") : e.msg;
      } catch (std::exception& e) {
        a.err = std::string("internal error: ") + e.what();
      }
      ahead = std::move(a);
    });
  }
  /* the next piece with at least one block, or false at the end of the input */
  bool next(Dev& d, MafInput& in) {
    for (;;) {
      if (!started) {
        started = true;
        read_ahead();
      }
      if (!reader.joinable()) return false; /* the end was seen */
      reader.join();
      Ahead a = std::move(ahead);
      if (!a.err.empty()) fail(a.err);
      if (!a.ok) return false;
      if (in.text && in.text.use_count() == 1) rd.recycle(std::move(*in.text)); /* nobody else holds the piece the caller is done with */
      read_ahead();
      if (on_piece) on_piece(a.text);
      in = maf_from_text(d, std::move(a.text), keep_going);
      if (first_seen) header = in.header;
      first_seen = false;
      if (!in.recs.empty() || !in.error.empty()) return true;
      if (in.d_text) d.release(in.d_text);
    }
  }
};

/* the (target row, query row) pairs of a list of blocks on the device: offsets into the uploaded file, or
 * — host reader — into one buffer the rows are gathered in */
struct MafRows {
  const uint8_t* d_rows = nullptr;
  uint64_t *d_t = nullptr, *d_q = nullptr, *d_c = nullptr;
  uint8_t* d_s = nullptr;
  std::vector<uint64_t> cols;
  bool names_in_rows = false; /* d_rows is the uploaded file: MafSLine::name_off points into its n_row_bytes bytes */
  uint64_t n_row_bytes = 0;
};
MafRows device_rows(Dev& d, const MafInput& in, const std::vector<const MafRecord*>& recs, bool cols_target) {
  MafRows m;
  std::vector<uint64_t> t_off, q_off;
  std::vector<uint8_t> strand;
  std::string blob;
  for (const MafRecord* r : recs) {
    const MafSLine &t = r->t(), &q = r->q();
    if (in.on_device) {
      t_off.push_back(t.seq_off);
      q_off.push_back(q.seq_off);
    } else {
      t_off.push_back(blob.size());
      blob.append(t.seq_data(), t.seq_size());
      q_off.push_back(blob.size());
      blob.append(q.seq_data(), q.seq_size());
    }
    /* zip truncates to the shorter row; `call` walks the target row's length (caller.rs:115) */
    m.cols.push_back(cols_target ? t.seq_size() : std::min(t.seq_size(), q.seq_size()));
    strand.push_back(q.neg ? 1 : 0);
  }
  d.init();
  m.d_rows = in.on_device ? in.d_text : d.upload((const uint8_t*)blob.data(), blob.size());
  m.names_in_rows = in.on_device;
  m.n_row_bytes = in.on_device ? in.text->size() : blob.size();
  m.d_t = d.upload(t_off);
  m.d_q = d.upload(q_off);
  m.d_c = d.upload(m.cols);
  m.d_s = d.upload(strand);
  return m;
}
std::vector<const MafRecord*> all_records(const std::vector<MafRecord>& recs) {
  std::vector<const MafRecord*> v;
  v.reserve(recs.size());
  for (const auto& r : recs) v.push_back(&r);
  return v;
}
/* --gpus N for the MAF commands: blocks are independent, so the selected blocks of a piece are dealt out in N contiguous
 * ranges; device 0 reads the rows where the piece was uploaded, the others get a gathered copy of their range's rows.
 * fn(g, dev, rows, lo, count) runs on one thread per device; results are merged by the caller in block order. */
struct MafDevices {
  Dev& d0;
  std::vector<std::unique_ptr<Dev>> extra;
  explicit MafDevices(Dev& first) : d0(first) {
    for (int g = 1; g < g_gpus; g++) extra.emplace_back(new Dev(g));
  }
  int count() const { return 1 + (int)extra.size(); }
  Dev& dev(int g) { return g == 0 ? d0 : *extra[g - 1]; }
  void release_all() {
    if (d0.ctx) d0.release_all();
    for (auto& e : extra)
      if (e->ctx) e->release_all(); /* a device that got no block of this piece was never started */
  }
  void run(const MafInput& in, const std::vector<const MafRecord*>& recs, bool cols_target,
           const std::function<void(int, Dev&, const MafRows&, uint32_t, uint32_t)>& fn) {
    const uint32_t n = (uint32_t)recs.size();
    const int ng = count();
    if (ng == 1) {
      MafRows p = device_rows(d0, in, recs, cols_target);
      fn(0, d0, p, 0, n);
      return;
    }
    on_devices(ng, [&](int g) {
      const uint32_t lo = (uint32_t)((uint64_t)n * g / ng), hi = (uint32_t)((uint64_t)n * (g + 1) / ng);
      if (lo == hi) return;
      std::vector<const MafRecord*> part(recs.begin() + lo, recs.begin() + hi);
      MafInput host_view; /* rows gathered from the host copy of the text */
      MafRows p = device_rows(dev(g), g == 0 ? in : host_view, part, cols_target);
      fn(g, dev(g), p, lo, hi - lo);
    });
  }
};

void select_query(std::vector<MafRecord>& recs, const std::string* query_name) {
  for (auto& r : recs) {
    if (query_name) { /* maf.rs:277-285 */
      size_t k = 0;
      for (; k < r.slines.size(); k++)
        if (r.slines[k].name == *query_name) break;
      if (k == r.slines.size()) fail("Query name:" + *query_name + " not found in MAF");
      r.query_idx = k;
    }
    if (r.query_idx >= r.slines.size())
      fail("panic: MAF block with a single s-line has no query row (maf.rs:426 index out of bounds)");
  }
}

int cmd_stat_maf(const std::string* input, bool each, const std::string* query_name, Output& out) {
  Dev d;
  MafDevices md(d);
  MafChunks chunks(input);
  std::vector<StatInput> in;
  MafInput min;
  while (chunks.next(d, min)) { /* one piece of the file at a time; only the per-block statistics are kept */
    std::vector<MafRecord>& recs = min.recs;
    select_query(recs, query_name);
    const uint32_t n = (uint32_t)recs.size();
    std::vector<wga_cigar_counts> counts(n);
    md.run(min, all_records(recs), false, [&](int, Dev& dg, const MafRows& p, uint32_t lo, uint32_t cnt) {
      auto* d_counts = (wga_cigar_counts*)dg.alloc((size_t)cnt * sizeof(wga_cigar_counts));
      auto* d_cnt = (uint64_t*)dg.alloc((size_t)cnt * 8);
      dg.check(wga_maf_pair_stat(dg.ctx, cnt, p.d_rows, p.d_t, p.d_q, p.d_c, p.d_s, d_counts, d_cnt, nullptr, nullptr));
      dg.download(counts.data() + lo, d_counts, cnt);
    });
    for (uint32_t k = 0; k < n; k++) {
      const MafRecord& r = recs[k];
      in.push_back(StatInput{r.t().name, r.q().name, r.t().size, r.q().size, r.t().start, r.query_start(),
                             recstat_from(counts[k])});
    }
    md.release_all();
  }
  out.write(stat_tsv(in, each));
  out.close();
  return leave(0);
}
