/* cmd_common.inc — part of wgatools_main.cpp (included there, inside its namespace, in front of the commands): what more than one
 * command does the same way.  The worker threads and devices of --gpus N, the single-device tokeniser + K1 step, the MAF input
 * and its rows on the device, K3's run list and the ops made of it, the heads the record writers take, the host's text
 * around text the device writes (WGA_*_WRITER=host), the download through the pinned buffers, and the rows of `stat --each`
 * (K33's heads, the pieces' texts and their order). */
/* one thread per device over fn(g); the first worker error (by device number) is rethrown on the caller's thread */
static void on_devices(int ngpu, const std::function<void(int)>& fn) {
  std::vector<std::string> werr(ngpu);
  std::vector<std::thread> th;
  for (int g = 0; g < ngpu; g++)
    th.emplace_back([&, g] {
      try {
        fn(g);
      } catch (Error& e) {
        werr[g] = e.msg.empty() ? std::string("error") : e.msg;
      } catch (std::exception& e) {
        werr[g] = std::string("internal error: ") + e.what();
      }
    });
  for (auto& t : th) t.join();
  for (int g = 0; g < ngpu; g++)
    if (!werr[g].empty()) fail(werr[g]);
}

/* --gpus N for the PAF and chain commands: one Dev per device, built on first use.  Device 0's worker borrows the reader's
 * context (the piece was uploaded and split there), the others own theirs. */
struct WorkerDevices {
  Dev& reader;
  std::vector<std::unique_ptr<Dev>> devs;
  explicit WorkerDevices(Dev& d) : reader(d) {}
  /* borrow = false: nothing of the input stands on device 0, its worker gets a context of its own */
  std::vector<std::unique_ptr<Dev>>& list(bool borrow = true) {
    if (devs.empty()) {
      for (int g = 0; g < g_gpus; g++) devs.emplace_back(new Dev(g));
      if (borrow) {
        devs[0]->ctx = reader.ctx;
        devs[0]->own_ctx = false;
      }
    }
    return devs;
  }
  /* fn(g, dev, lo, hi, d_text_here) on one thread per device over contiguous ranges [lo, hi) of a piece's records.  A piece
   * that was split on the device has its text uploaded to the other devices (d_text_here, else nullptr); what a worker
   * allocates is released behind fn.  The caller joins the devices' results in device order. */
  void run(const PafInput& pin, const std::function<void(int, Dev&, size_t, size_t, const uint8_t*)>& fn) {
    reader.init();
    list();
    const int ng = (int)devs.size();
    const size_t n = pin.recs.size();
    std::string text16;
    if (pin.on_device) text16 = pin.text + std::string(16, '\0');
    on_devices(ng, [&](int g) {
      const size_t lo = n * (size_t)g / ng, hi = n * (size_t)(g + 1) / ng;
      if (lo == hi) return;
      Dev& dg = *devs[g];
      dg.init();
      const size_t keep = dg.owned.size();
      const uint8_t* d_text = nullptr;
      if (pin.on_device) d_text = g == 0 ? pin.d_text : dg.upload((const uint8_t*)text16.data(), text16.size());
      fn(g, dg, lo, hi, d_text);
      dg.release_to(keep);
    });
  }
};

/* the reference's message for an op K1 rejects */
static std::string bad_op_message(const CigarTexts& cigars, size_t k, const wga_rec_diag& g) {
  return "CIGAR OP `" + cigar_op_token_at(cigars[k], g.bad_op_idx) + "` invalid";
}
/* Records [0, n) of a piece on one device: tokeniser, then K1 over the records in front of the first tag / tokeniser error; their
 * counts come back.  Returns that error's message and sets op_err to the message for the first op K1 rejects ("" if none): which
 * of the two speaks, and how, is the command's.  on_device: the counts are not downloaded, *on_device is where they stand. */
static std::string paf_counts(Dev& d, const PafInput& pin, uint32_t n, std::vector<wga_cigar_counts>& counts, std::string& op_err,
                              const wga_cigar_counts** on_device = nullptr) {
  CigarTexts cigars;
  wga_cigar_batch cb;
  const std::string e = device_tokenise(d, pin, 0, n, cigars, &cb);
  const uint32_t m = cb.n;
  if (on_device) *on_device = nullptr;
  if (m) {
    auto* d_counts = (wga_cigar_counts*)d.alloc((size_t)m * sizeof(wga_cigar_counts));
    auto* d_diag = (wga_rec_diag*)d.alloc((size_t)m * sizeof(wga_rec_diag));
    d.check(wga_cigar_stat(d.ctx, &cb, d_counts, d_diag, nullptr));
    std::vector<wga_rec_diag> diag(m);
    d.download(diag.data(), d_diag, m);
    if (on_device) *on_device = d_counts; /* the counts stay where K1 left them (stat -e: K33 reads them there) */
    else d.download(counts.data(), d_counts, m);
    for (uint32_t k = 0; k < m && op_err.empty(); k++)
      if (diag[k].bad_op_idx != WGA_NONE) op_err = bad_op_message(cigars, k, diag[k]);
  }
  return e;
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
  wga_maf_line* d_lines = nullptr; /* lines_only: the splitter's table stays on the device, n_lines entries; no records are built */
  uint64_t n_lines = 0;
};
/* lines_only (maf-index): a piece the device splitter can be asked about keeps its line table on the device and gets no host
 * records — the table is not even looked at here, so a WGA_MAF_FALLBACK line in it is the caller's to find (wga_maf_index
 * refuses such a table) and to read with parse_maf. */
MafInput maf_from_text(Dev& d, std::string&& whole_text, bool keep_going = false, bool lines_only = false) {
  MafInput in;
  *in.text = std::move(whole_text);
  const std::string& text = *in.text;
  /* WGA_MAF_READER=host: always the host reader (measurements) */
  if (!text.empty() && text.size() < 0xFFFFFFF0ull && !env_is("WGA_MAF_READER", "host")) {
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
    if (lines_only) {
      g_timer.mark("device split");
      in.on_device = true;
      in.d_lines = d_lines;
      in.n_lines = n_lines;
      size_t he = text.find('\n');
      if (he == std::string::npos) he = text.size();
      if (he > 0 && text[he - 1] == '\r') he--;
      in.header.assign(text, 0, he);
      return in;
    }
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
  bool lines_only = false; /* maf-index: next() hands out EVERY piece, a device-split one with its line table and without records */
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
      in = maf_from_text(d, std::move(a.text), keep_going, lines_only);
      if (first_seen) header = in.header;
      first_seen = false;
      if (lines_only || !in.recs.empty() || !in.error.empty()) return true;
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

/* K3's run list for the blocks of `p` on device d: the count call (the blocks' counts and their numbers of runs), the scan, the
 * fill call.  counts_only stops behind the count call. */
struct MafRuns {
  wga_cigar_counts* d_counts = nullptr;
  uint64_t *d_cnt = nullptr, *d_roff = nullptr, *d_runs = nullptr;
  uint64_t n_runs = 0;
};
static MafRuns maf_runs(Dev& d, const MafRows& p, uint32_t n, bool counts_only = false) {
  MafRuns r;
  r.d_counts = (wga_cigar_counts*)d.alloc((size_t)n * sizeof(wga_cigar_counts));
  r.d_cnt = (uint64_t*)d.alloc((size_t)n * 8);
  d.check(wga_maf_pair_stat(d.ctx, n, p.d_rows, p.d_t, p.d_q, p.d_c, p.d_s, r.d_counts, r.d_cnt, nullptr, nullptr));
  if (counts_only) return r;
  r.d_roff = d.scan(n, r.d_cnt, &r.n_runs);
  r.d_runs = (uint64_t*)d.alloc((r.n_runs + 1) * 8);
  d.check(wga_maf_pair_stat(d.ctx, n, p.d_rows, p.d_t, p.d_q, p.d_c, p.d_s, r.d_counts, r.d_cnt, r.d_runs, r.d_roff));
  return r;
}
/* ... and the runs as packed ops (wga_maf_runs_ops: count, scan, fill): the batch the CIGAR kernels take */
static wga_cigar_batch maf_runs_batch(Dev& d, const MafRows& p, uint32_t n, const MafRuns& r) {
  wga_cigar_batch cb;
  auto* d_ocnt = (uint64_t*)d.alloc((size_t)n * 8);
  d.check(wga_maf_runs_ops(d.ctx, n, r.n_runs, r.d_runs, r.d_roff, p.d_c, d_ocnt, nullptr, nullptr));
  uint64_t* d_ooff = d.scan(n, d_ocnt, &cb.n_ops);
  auto* d_ops = (uint32_t*)d.alloc((cb.n_ops + 4) * 4);
  d.check(wga_maf_runs_ops(d.ctx, n, r.n_runs, r.d_runs, r.d_roff, p.d_c, nullptr, d_ops, d_ooff));
  cb.d_ops = d_ops;
  cb.d_op_off = d_ooff;
  cb.d_strand_neg = p.d_s;
  cb.n = n;
  return cb;
}

/* The heads the record writers take (wga_maf2paf, wga_chain_heads): a record's numbers and where its two names stand — in the
 * uploaded file where the device splitter took the piece and this device holds it (MafRows::names_in_rows), otherwise in a
 * buffer the names are gathered in, query name first. */
static wga_maf2paf_head record_head(uint64_t q_size, uint64_t q_start, uint64_t q_end, bool neg, uint64_t t_size, uint64_t t_start,
                                    uint64_t t_end) {
  wga_maf2paf_head h;
  memset(&h, 0, sizeof h);
  h.q[0] = q_size, h.q[1] = q_start, h.q[2] = q_end;
  h.t[0] = t_size, h.t[1] = t_start, h.t[2] = t_end;
  h.strand_neg = neg ? 1 : 0;
  return h;
}
static wga_maf2paf_head record_head(const MafRecord& r) {
  return record_head(r.q().size, r.query_start(), r.query_end(), r.q().neg, r.t().size, r.t().start, r.t().start + r.t().align_size);
}
static wga_maf2paf_head record_head(const PafRecord& r) {
  return record_head(r.query_length, r.query_start, r.query_end, r.neg, r.target_length, r.target_start, r.target_end);
}
/* The names a batch's heads point into: in the uploaded file where the device splitter took the piece and this device holds it
 * (rows), otherwise gathered here once per batch and uploaded (RecordHeads below, MafFrameHeads of paf2maf and chain2maf). */
struct NameSpans {
  std::string names;
  const MafRows* rows; /* the uploaded rows the names are read in, or nullptr: gathered */
  const uint8_t* d_names = nullptr;
  uint64_t n_name_bytes = 0;
  explicit NameSpans(const MafRows* p = nullptr) : rows(p && p->names_in_rows ? p : nullptr) {}
  void span(const std::string& name, uint64_t at_in_rows, uint64_t& off, uint32_t& len) {
    off = rows ? at_in_rows : names.size();
    len = (uint32_t)name.size();
    if (!rows) names += name;
  }
  void upload_names(Dev& d) {
    d_names = rows ? rows->d_rows : d.upload((const uint8_t*)names.data(), names.size());
    n_name_bytes = rows ? rows->n_row_bytes : names.size();
  }
};
struct RecordHeads : NameSpans {
  std::vector<wga_maf2paf_head> heads;
  const wga_maf2paf_head* d_heads = nullptr;
  explicit RecordHeads(uint32_t n, const MafRows* p = nullptr) : NameSpans(p) { heads.reserve(n); }
  void add(const MafRecord& r) {
    wga_maf2paf_head h = record_head(r);
    span(r.q().name, r.q().name_off, h.qname_off, h.qname_len);
    span(r.t().name, r.t().name_off, h.tname_off, h.tname_len);
    heads.push_back(h);
  }
  void add(const PafRecord& r) {
    wga_maf2paf_head h = record_head(r);
    span(r.query_name, 0, h.qname_off, h.qname_len);
    span(r.target_name, 0, h.tname_off, h.tname_len);
    heads.push_back(h);
  }
  void upload(Dev& d) {
    upload_names(d);
    d_heads = d.upload(heads);
  }
};

/* Host text around device text (the host writers of WGA_*_WRITER=host): every record is a head from the host, a middle a kernel
 * writes at mid_off[k], a tail from the host.  Heads and tails stand back to back in `blob`; scatter() drops them into the
 * output around the middles (wga_scatter_bytes). */
struct HostFraming {
  std::string blob;
  std::vector<uint64_t> blob_off{0}, dst, mid_off;
  uint64_t pos = 0; /* the text's length so far */
  /* the next record: `head` and `tail` bytes of the blob (a caller that fills the blob itself) around `middle` bytes */
  void place(uint64_t head, uint64_t middle, uint64_t tail) {
    dst.push_back(pos);
    blob_off.push_back(blob_off.back() + head);
    pos += head;
    mid_off.push_back(pos);
    pos += middle;
    dst.push_back(pos);
    blob_off.push_back(blob_off.back() + tail);
    pos += tail;
  }
  void add(const std::string& head, uint64_t middle, const char* tail) {
    blob += head;
    blob += tail;
    place(head.size(), middle, strlen(tail));
  }
  void scatter(Dev& d, uint8_t* d_out) {
    auto* d_blob = d.upload((const uint8_t*)blob.data(), blob.size());
    auto *d_blob_off = d.upload(blob_off), *d_dst = d.upload(dst);
    d.check(wga_scatter_bytes(d.ctx, (uint32_t)dst.size(), d_blob, d_blob_off, d_out, d_dst));
  }
};

/* a chain's head line without its line end (chain.rs:103-140,142-203), the alignment's ends moved in by the trims */
static void append_chain_head(std::string& s, const std::string& t_name, uint64_t t_size, uint64_t t_start, uint64_t t_end,
                              const std::string& q_name, uint64_t q_size, bool neg, uint64_t q_start, uint64_t q_end,
                              const wga_chain_trim_t& trim, uint64_t id) {
  t_start += trim.head_del;
  t_end -= trim.tail_del;
  if (!neg) {
    q_start += trim.head_ins;
    q_end -= trim.tail_ins;
  } else { /* chain.rs:131-136: the new end is computed from the already updated start */
    q_start = q_size - (q_end - trim.head_ins);
    q_end = q_size - (q_start + trim.tail_ins);
  }
  s += "chain\t255\t" + t_name + "\t";
  append_u64(s, t_size);
  s += "\t+\t";
  append_u64(s, t_start);
  s.push_back('\t');
  append_u64(s, t_end);
  s += "\t" + q_name + "\t";
  append_u64(s, q_size);
  s += neg ? "\t-\t" : "\t+\t";
  append_u64(s, q_start);
  s.push_back('\t');
  append_u64(s, q_end);
  s.push_back('\t');
  append_u64(s, id);
}

/* the twelve columns of a PAF line as the csv writer gives them (paf.rs:50-65) */
static void append_paf_columns(std::string& s, const std::string& q_name, uint64_t q_size, uint64_t q_start, uint64_t q_end, bool neg,
                               const std::string& t_name, uint64_t t_size, uint64_t t_start, uint64_t t_end, uint64_t matches,
                               uint64_t block, uint64_t mapq = 255) {
  append_csv_field(s, q_name, '\t');
  for (uint64_t v : {q_size, q_start, q_end}) {
    s.push_back('\t');
    append_u64(s, v);
  }
  s += neg ? "\t-\t" : "\t+\t";
  append_csv_field(s, t_name, '\t');
  for (uint64_t v : {t_size, t_start, t_end, matches, block, mapq}) {
    s.push_back('\t');
    append_u64(s, v);
  }
}

/* n bytes of device memory behind `dst`: two pinned buffers, the copy of one slab runs while the one before it is appended */
static void download_append(Dev& d, std::string& dst, const uint8_t* d_src, size_t n) {
  if (n == 0) return;
  if (!d.streamer) d.streamer.reset(new DevStreamer(d.ctx));
  DevStreamer& st = *d.streamer;
  for (int k = 0; k < 2; k++)
    if (!st.buf[k] && wga_host_alloc(d.ctx, DevStreamer::kPiece, &st.buf[k])) fail(std::string("GPU engine: ") + wga_last_error());
  dst.reserve(dst.size() + n);
  const size_t kPiece = DevStreamer::kPiece, np = (n + kPiece - 1) / kPiece;
  d.check(wga_memcpy_d2h_async(d.ctx, st.buf[0], d_src, std::min(kPiece, n)));
  for (size_t p = 0; p < np; p++) {
    d.check(wga_sync(d.ctx));
    if (p + 1 < np) d.check(wga_memcpy_d2h_async(d.ctx, st.buf[(p + 1) & 1], d_src + (p + 1) * kPiece, std::min(kPiece, n - (p + 1) * kPiece)));
    dst.append((const char*)st.buf[p & 1], std::min(kPiece, n - p * kPiece));
  }
}

/* The two calls of a text entry: call(d_work, &bytes, d_out) counts with d_out == nullptr and writes the text otherwise.  The
 * work area is work_bytes long (the entry's own plus what the site asks for behind it), the output has 64 bytes of slack behind
 * the text; the fill call at zero bytes is made only where fill_empty says so.  Both areas stay the caller's to release. */
struct DevText {
  void* d_work;
  uint8_t* d_out;
  size_t bytes;
};
static DevText two_call_text(Dev& d, size_t work_bytes, const std::function<int(void*, uint64_t*, uint8_t*)>& call,
                             bool fill_empty = false) {
  void* d_work = d.alloc(work_bytes);
  uint64_t bytes = 0;
  d.check(call(d_work, &bytes, nullptr));
  auto* d_out = (uint8_t*)d.alloc((size_t)bytes + 64);
  if (bytes || fill_empty) d.check(call(d_work, &bytes, d_out));
  return {d_work, d_out, (size_t)bytes};
}

/* The rows of a row writer (K33, K34) for the records of hd (heads of type Head: the rest of hd), appended to `text`:
 * call(d_heads, d_work, d_row_off, &bytes, d_out) is the entry.  Returns the rows' offsets on the device, n + 1. */
template <typename Head, typename Call>
static const uint64_t* record_rows_text(Dev& d, NameSpans& hd, const std::vector<Head>& heads, size_t work_bytes, std::string& text,
                                        const Call& call) {
  hd.upload_names(d);
  const Head* d_heads = d.upload(heads);
  auto* d_off = (uint64_t*)d.alloc((heads.size() + 1) * 8);
  const DevText t = two_call_text(
      d, work_bytes, [&](void* d_work, uint64_t* bytes, uint8_t* d_out) { return call(d_heads, d_work, d_off, bytes, d_out); });
  download_append(d, text, t.d_out, t.bytes);
  return d_off;
}

/* ---- stat --each on the device (K33, wga_stat_rows) ------------------------------------------------------------------------------
 * WGA_STAT_WRITER=host: stat_tsv builds, sorts and prints a Statistic per record on one host thread, as before K33 (measurements,
 * and the cross-check of the device writer: same bytes) */
static bool stat_host_writer() { return env_is("WGA_STAT_WRITER", "host"); }

/* the heads wga_stat_rows takes: a record's four numbers and where its two names stand (NameSpans) */
struct StatRowHeads : NameSpans {
  std::vector<wga_stat_row_head> heads;
  explicit StatRowHeads(uint32_t n, const MafRows* p = nullptr) : NameSpans(p) { heads.reserve(n); }
  void add(const std::string& ref_name, uint64_t ref_at, uint64_t ref_size, uint64_t ref_start, const std::string& query_name,
           uint64_t query_at, uint64_t query_size, uint64_t query_start) {
    wga_stat_row_head h;
    h.ref_size = ref_size, h.ref_start = ref_start, h.query_size = query_size, h.query_start = query_start;
    span(ref_name, ref_at, h.rname_off, h.rname_len);
    span(query_name, query_at, h.qname_off, h.qname_len);
    heads.push_back(h);
  }
};

/* The rows of `stat --each` over all pieces.  A piece's rows are written on the device in input order and come back as one text
 * with its row offsets; of a record the host keeps only the id of its distinct ref_name.  The rows leave sorted stably by the
 * natural order of ref_name (stat.rs:104): the DISTINCT names are sorted with natord_compare, names that compare equal (natord
 * skips white space: "c 1" and "c1") share a rank, and a stable counting sort on the rank orders the records — the order of a
 * stable_sort over all records, for n log n fewer string comparisons. */
struct StatRows {
  std::vector<std::string> text;              /* per piece */
  std::vector<std::vector<uint64_t>> row_off; /* per piece: n + 1 */
  std::vector<uint32_t> name_id;              /* per record, over all pieces */
  std::unordered_map<std::string, uint32_t> ids;
  std::vector<const std::string*> distinct; /* the keys of `ids` (node addresses are stable) */
  const std::string* last = nullptr;
  uint32_t last_id = 0;
  void note(const std::string& ref_name) {
    if (!last || *last != ref_name) { /* neighbours mostly share their target */
      auto it = ids.find(ref_name);
      if (it == ids.end()) {
        it = ids.emplace(ref_name, (uint32_t)distinct.size()).first;
        distinct.push_back(&it->first);
      }
      last = &it->first;
      last_id = it->second;
    }
    name_id.push_back(last_id);
  }
  /* the rows of the n records noted last, whose counts stand on d (device 0) */
  void piece(Dev& d, StatRowHeads& hd, const wga_cigar_counts* d_counts) {
    const uint32_t n = (uint32_t)hd.heads.size();
    text.emplace_back();
    const uint64_t* d_off = record_rows_text(
        d, hd, hd.heads, (size_t)wga_stat_rows_work_bytes(n), text.back(),
        [&](const wga_stat_row_head* d_heads, void* d_work, uint64_t* d_row_off, uint64_t* total, uint8_t* d_out) {
          return wga_stat_rows(d.ctx, n, hd.d_names, hd.n_name_bytes, d_heads, d_counts, d_work, d_row_off, total, d_out);
        });
    std::string offs; /* the offsets through the same pinned buffers */
    download_append(d, offs, (const uint8_t*)d_off, ((size_t)n + 1) * 8);
    row_off.emplace_back((size_t)n + 1);
    memcpy(row_off.back().data(), offs.data(), offs.size());
    g_timer.mark("stat rows (device)");
  }
  /* the header (only in front of a row: the csv writer prints it with the first record) and the rows in their order */
  void write(Output& out) {
    const size_t n_rows = name_id.size();
    if (n_rows == 0) return;
    const uint32_t nd = (uint32_t)distinct.size();
    std::vector<uint32_t> order(nd), rank(nd);
    for (uint32_t k = 0; k < nd; k++) order[k] = k;
    std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return natord_compare(*distinct[a], *distinct[b]) < 0; });
    uint32_t n_rank = 0;
    for (uint32_t k = 0; k < nd; k++) {
      if (k && natord_compare(*distinct[order[k - 1]], *distinct[order[k]]) < 0) n_rank++;
      rank[order[k]] = n_rank;
    }
    n_rank++;
    std::vector<size_t> at(n_rank + 1, 0); /* counting sort: where a rank's rows begin */
    for (uint32_t id : name_id) at[rank[id] + 1]++;
    for (uint32_t k = 0; k < n_rank; k++) at[k + 1] += at[k];
    std::vector<uint64_t> rows(n_rows); /* piece << 32 | row in the piece */
    size_t g = 0;
    for (size_t p = 0; p < text.size(); p++)
      for (size_t k = 0; k + 1 < row_off[p].size(); k++, g++) rows[at[rank[name_id[g]]]++] = (uint64_t)p << 32 | (uint64_t)k;
    std::string buf =
        "ref_name\tref_size\tref_start\tquery_name\tquery_size\tquery_start\taligned_size\t"
        "unaligned_size\tidentity\tsimilarity\tmatched\tmismatched\tins_event\tdel_event\tins_size\t"
        "del_size\tinv_event\tinv_size\tinv_ins_event\tinv_ins_size\tinv_del_event\tinv_del_size\n";
    const size_t kFlush = (size_t)8 << 20;
    buf.reserve(kFlush + 4096);
    for (uint64_t r : rows) {
      const size_t p = (size_t)(r >> 32), k = (size_t)(r & 0xFFFFFFFFu);
      buf.append(text[p], (size_t)row_off[p][k], (size_t)(row_off[p][k + 1] - row_off[p][k]));
      if (buf.size() >= kFlush) {
        out.write(buf);
        buf.clear();
      }
    }
    out.write(buf);
    g_timer.mark("stat rows gathered + written");
  }
};

/* ---- stat's merged table on the device (K36, wga_stat_pairs and wga_stat_pair_rows) -------------------------------------------------
 * Per piece the device groups the records into pairs (ref_name, ref_size, query_name, query_size), sums the counters and folds
 * inv_size; only the piece's pairs come back.  The host keeps ONE table of global pairs in first-appearance order — a map over
 * pairs, not records, looked up through the head of a piece pair's first record — adds the piece's sums mod 2^64 and takes the
 * minima.  inv_size is an f32 sum in record order (stat.rs:206), so a pair that already carries a non-zero value and gets
 * inverted records again has its fold repeated from the carried value (the second call again, with d_inv_in).  After the last
 * piece the pairs are ordered stably by the natural order of ref_name (stat.rs:116) and their rows are written on the device.
 * WGA_STAT_WRITER=host keeps stat_tsv's path. */
struct StatTable {
  struct Pair {
    std::string ref_name, query_name;
    uint64_t ref_size, query_size, ref_start, query_start;
    wga_cigar_counts sum;
    uint32_t inv_bits;
  };
  std::vector<Pair> pairs; /* first-appearance order */
  std::map<std::tuple<std::string, uint64_t, std::string, uint64_t>, size_t> index;
  /* the n records of hd, whose counts stand on d; names_of(k) = record k's (ref_name, query_name) */
  template <typename NamesOf>
  void piece(Dev& d, StatRowHeads& hd, const wga_cigar_counts* d_counts, const NamesOf& names_of) {
    const uint32_t n = (uint32_t)hd.heads.size();
    if (n == 0) return;
    hd.upload_names(d);
    const wga_stat_row_head* d_heads = d.upload(hd.heads);
    void* d_work = d.alloc((size_t)wga_stat_pairs_work_bytes(n));
    uint64_t np = 0;
    d.check(wga_stat_pairs(d.ctx, n, hd.d_names, hd.n_name_bytes, d_heads, d_counts, d_work, &np, nullptr, nullptr, nullptr, 0));
    auto* d_por = (uint32_t*)d.alloc((size_t)n * 4);
    auto* d_pairs = (wga_stat_pair*)d.alloc((size_t)np * sizeof(wga_stat_pair));
    d.check(wga_stat_pairs(d.ctx, n, hd.d_names, hd.n_name_bytes, d_heads, d_counts, d_work, &np, d_por, nullptr, d_pairs, np));
    std::vector<wga_stat_pair> got((size_t)np);
    d.download(got.data(), d_pairs, (size_t)np);
    std::vector<size_t> global((size_t)np);
    std::vector<uint32_t> carried((size_t)np);
    bool refold = false;
    for (size_t p = 0; p < (size_t)np; p++) {
      if (got[p].first_rec >= n) fail("GPU engine: a pair's first record lies outside the piece");
      const wga_stat_row_head& H = hd.heads[(size_t)got[p].first_rec];
      const auto names = names_of((size_t)got[p].first_rec);
      auto key = std::make_tuple(*names.first, H.ref_size, *names.second, H.query_size);
      auto it = index.find(key);
      if (it == index.end()) {
        Pair q;
        q.ref_name = *names.first, q.query_name = *names.second;
        q.ref_size = q.ref_start = H.ref_size; /* minima start from the sizes, stat.rs:186,189 */
        q.query_size = q.query_start = H.query_size;
        memset(&q.sum, 0, sizeof q.sum);
        q.inv_bits = 0;
        it = index.emplace(std::move(key), pairs.size()).first;
        pairs.push_back(std::move(q));
      }
      global[p] = it->second;
      carried[p] = pairs[it->second].inv_bits;
      /* a fold from +0.0 that is not +0.0: the piece adds something to this pair's inv_size */
      if (got[p].inv_size_bits != 0 && carried[p] != 0) refold = true;
    }
    if (refold) { /* rare: the folds again, from what the pairs carry */
      const uint32_t* d_inv = d.upload(carried);
      d.check(wga_stat_pairs(d.ctx, n, hd.d_names, hd.n_name_bytes, d_heads, d_counts, d_work, &np, d_por, d_inv, d_pairs, np));
      d.download(got.data(), d_pairs, (size_t)np);
    }
    for (size_t p = 0; p < (size_t)np; p++) {
      Pair& q = pairs[global[p]];
      const uint64_t* a = (const uint64_t*)&got[p].sum;
      uint64_t* b = (uint64_t*)&q.sum;
      for (int k = 0; k < 11; k++) b[k] += a[k];
      q.ref_start = std::min(q.ref_start, got[p].ref_start);
      q.query_start = std::min(q.query_start, got[p].query_start);
      if (refold || got[p].inv_size_bits != 0) q.inv_bits = got[p].inv_size_bits;
    }
    g_timer.mark("stat table (device)");
  }
  /* the header (only in front of a row) and the rows */
  void write(Dev& d, Output& out) {
    const uint32_t n = (uint32_t)pairs.size();
    if (n == 0) return;
    std::vector<uint32_t> order(n);
    for (uint32_t k = 0; k < n; k++) order[k] = k;
    std::stable_sort(order.begin(), order.end(),
                     [&](uint32_t a, uint32_t b) { return natord_compare(pairs[a].ref_name, pairs[b].ref_name) < 0; });
    d.init();
    StatRowHeads hd(n);
    std::vector<wga_cigar_counts> sums;
    std::vector<uint32_t> inv;
    sums.reserve(n), inv.reserve(n);
    for (uint32_t k : order) {
      const Pair& q = pairs[k];
      hd.add(q.ref_name, 0, q.ref_size, q.ref_start, q.query_name, 0, q.query_size, q.query_start);
      sums.push_back(q.sum);
      inv.push_back(q.inv_bits);
    }
    const wga_cigar_counts* d_sums = d.upload(sums);
    const uint32_t* d_inv = d.upload(inv);
    std::string text =
        "ref_name\tref_size\tref_start\tquery_name\tquery_size\tquery_start\taligned_size\t"
        "unaligned_size\tidentity\tsimilarity\tmatched\tmismatched\tins_event\tdel_event\tins_size\t"
        "del_size\tinv_event\tinv_size\tinv_ins_event\tinv_ins_size\tinv_del_event\tinv_del_size\n";
    record_rows_text(d, hd, hd.heads, (size_t)wga_stat_rows_work_bytes(n), text,
                     [&](const wga_stat_row_head* d_heads, void* d_work, uint64_t* d_row_off, uint64_t* total, uint8_t* d_out) {
                       return wga_stat_pair_rows(d.ctx, n, hd.d_names, hd.n_name_bytes, d_heads, d_sums, d_inv, d_work, d_row_off, total,
                                                 d_out);
                     });
    out.write(text);
    d.release_all();
    g_timer.mark("stat table (device)");
  }
};
