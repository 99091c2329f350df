/* cmd_chain.inc — part of wgatools_main.cpp (included there, inside its namespace: the commands share the device helpers, readers and
 * writers defined in front of the include). */
/* ---- paf2chain (converter.rs:148-173; SURVEY.md 8f rank 2) ------------------------------------------------
 * GPU: tokeniser, data lines and head / tail trims (wga_cigar_chain, K10), the chain headers (chain.rs:142-203, incl. the '-'
 * strand arithmetic that reuses the updated start), the "\n\n" behind a record and the layout (wga_chain_heads, K30).  Host: one
 * wga_maf2paf_head per record (the numbers of the PAF line, the spans of the two names) and the names gathered for the upload;
 * the length of the text, the number of records in front of the first bad one and that record's diagnostics come back.
 * WGA_CHAIN_HEAD_WRITER=host: the headers are printed by one host thread from the downloaded trims and scattered around the data
 * lines, as before K30 (measurements, and the cross-check of the device writer: same bytes); maf2chain below reads it too. */
static bool chain_head_host_writer() { return env_is("WGA_CHAIN_HEAD_WRITER", "host"); }
/* K10's count call over a batch: the trims, the data lines' bytes and the diagnostics of every record, on the device */
struct ChainTrims {
  wga_chain_trim_t* d_trim;
  uint64_t* d_nb;
  wga_rec_diag* d_diag;
};
static ChainTrims chain_trims(Dev& d, const wga_cigar_batch& cb) {
  ChainTrims t;
  t.d_trim = (wga_chain_trim_t*)d.alloc((size_t)cb.n * sizeof(wga_chain_trim_t));
  t.d_nb = (uint64_t*)d.alloc((size_t)cb.n * 8);
  t.d_diag = (wga_rec_diag*)d.alloc((size_t)cb.n * sizeof(wga_rec_diag));
  d.check(wga_cigar_chain(d.ctx, &cb, t.d_trim, t.d_nb, t.d_diag, nullptr, nullptr));
  return t;
}
/* the chain text of a batch whose K10 count call has run (t, on device d) and whose heads are uploaded (hd): K30's count call
 * lays the records out, K10's fill call writes the data lines of the records in front of the first bad one, K30's fill call the
 * heads and record ends around them.  Returns the text (on the device) and sets *bytes and *n_good. */
static const uint8_t* chain_text_device(Dev& d, const wga_cigar_batch& cb, const RecordHeads& hd, const ChainTrims& t,
                                        uint64_t chain_id0, uint64_t* bytes, uint32_t* n_good) {
  const uint32_t n = cb.n;
  void* d_work = d.alloc((size_t)wga_chain_heads_work_bytes(n));
  auto* d_data_off = (uint64_t*)d.alloc((size_t)n * 8);
  d.check(wga_chain_heads(d.ctx, n, hd.d_names, hd.n_name_bytes, hd.d_heads, t.d_trim, t.d_nb, t.d_diag, chain_id0, d_work,
                          d_data_off, bytes, n_good, nullptr));
  auto* d_out = (uint8_t*)d.alloc((size_t)*bytes + 64);
  if (*n_good) {
    wga_cigar_batch cb2 = cb;
    cb2.n = *n_good;
    d.check(wga_cigar_chain(d.ctx, &cb2, nullptr, nullptr, nullptr, d_out, d_data_off));
    d.check(wga_chain_heads(d.ctx, n, hd.d_names, hd.n_name_bytes, hd.d_heads, t.d_trim, t.d_nb, t.d_diag, chain_id0, d_work,
                            d_data_off, bytes, n_good, d_out));
  }
  return d_out;
}
/* ... and with the heads printed by the host: the data lines of records [0, f.mid_off.size()) between the heads and record ends
 * that were added to f */
static const uint8_t* chain_text_host(Dev& d, const wga_cigar_batch& cb, HostFraming& f) {
  auto* d_out = (uint8_t*)d.alloc(f.pos + 64);
  wga_cigar_batch cb2 = cb;
  cb2.n = (uint32_t)f.mid_off.size();
  d.check(wga_cigar_chain(d.ctx, &cb2, nullptr, nullptr, nullptr, d_out, d.upload(f.mid_off)));
  f.scatter(d, d_out);
  return d_out;
}
/* the chains of records [lo, hi) of a piece on device d, in resident batches; a batch's text goes to `sink` while it is still on
 * the device.  Returns the reference's message for the first failing record ("" if none): the records in front of it are written. */
static std::string paf2chain_range(Dev& d, const PafInput& pin, size_t lo, size_t hi, uint64_t chain_base,
                                   const uint8_t* d_text_here,
                                   const std::function<void(Dev&, const uint8_t*, size_t)>& sink) {
  const std::vector<PafRecord>& recs = pin.recs;
  const uint64_t kMaxText = 160ull << 20;
  const bool host_writer = chain_head_host_writer();
  std::string pending_error;
  const size_t keep = d.owned.size(); /* this piece's text */
  size_t i0 = lo;
  while (i0 < hi && pending_error.empty()) {
    size_t i = i0;
    uint64_t est_text = 0;
    for (; i < hi; i++) {
      if (i > i0 && est_text > kMaxText) break;
      est_text += pin.cigar_bytes(i);
    }
    d.init();
    CigarTexts cigars;
    wga_cigar_batch cb;
    pending_error = device_tokenise(d, pin, i0, (uint32_t)(i - i0), cigars, &cb, nullptr, nullptr, d_text_here);
    const uint32_t n = cb.n;
    if (n) {
      const ChainTrims t = chain_trims(d, cb);
      if (!host_writer) {
        RecordHeads hd(n);
        for (uint32_t k = 0; k < n; k++) hd.add(recs[i0 + k]);
        hd.upload(d);
        uint64_t bytes = 0;
        uint32_t good = 0;
        const uint8_t* d_out = chain_text_device(d, cb, hd, t, chain_base + (uint64_t)i0, &bytes, &good);
        if (good < n) { /* parse_cigar_to_trim fails before anything of the record is written */
          wga_rec_diag g;
          d.download(&g, t.d_diag + good, 1);
          pending_error = bad_op_message(cigars, good, g);
        }
        if (good) sink(d, d_out, (size_t)bytes);
      } else {
        std::vector<wga_chain_trim_t> trim(n);
        std::vector<uint64_t> nb(n);
        std::vector<wga_rec_diag> diag(n);
        d.download(trim.data(), t.d_trim, n);
        d.download(nb.data(), t.d_nb, n);
        d.download(diag.data(), t.d_diag, n);
        HostFraming f;
        for (uint32_t k = 0; k < n; k++) {
          if (diag[k].bad_op_idx != WGA_NONE) { /* parse_cigar_to_trim fails before anything of the record is written */
            pending_error = bad_op_message(cigars, k, diag[k]);
            break;
          }
          const PafRecord& r = recs[i0 + k];
          std::string h;
          append_chain_head(h, r.target_name, r.target_length, r.target_start, r.target_end, r.query_name, r.query_length, r.neg,
                            r.query_start, r.query_end, trim[k], chain_base + (uint64_t)(i0 + k));
          f.add(h, nb[k], "\n\n");
        }
        if (f.pos) sink(d, chain_text_host(d, cb, f), (size_t)f.pos);
      }
    }
    d.release_to(keep);
    i0 = i;
  }
  return pending_error;
}

int cmd_paf2chain(const std::string* input, Output& out) {
  Dev d;
  PafChunks chunks(input, false);
  std::string pending_error;
  PafInput pin;
  uint64_t chain_base = 0; /* chain id = index of the record in the whole input */
  const char* const records_phase = chain_head_host_writer() ? "paf2chain records (host)" : "paf2chain records (device)";
  WorkerDevices wd(d); /* --gpus N */
  for (;;) {
    bool more = false;
    try {
      more = chunks.next(d, pin);
    } catch (Error& e) {
      pending_error = e.msg;
    }
    if (!more) break;
    const size_t n = pin.recs.size();
    if (g_gpus == 1) {
      pending_error = paf2chain_range(d, pin, 0, n, chain_base, nullptr, [&](Dev& dg, const uint8_t* d_out, size_t bytes) {
        dg.check(wga_sync(dg.ctx));
        g_timer.mark(records_phase);
        stream_out(dg, out, d_out, bytes);
      });
      g_timer.mark(records_phase); /* a piece without a record to write */
    } else { /* a piece's records in contiguous ranges over the devices; the chains meet in input order, up to the first error */
      const int ng = g_gpus;
      std::vector<std::string> part(ng), err(ng);
      wd.run(pin, [&](int g, Dev& dg, size_t lo, size_t hi, const uint8_t* d_text) {
        err[g] = paf2chain_range(dg, pin, lo, hi, chain_base, d_text, [&](Dev& dd, const uint8_t* d_out, size_t bytes) {
          const size_t at = part[g].size();
          part[g].resize(at + bytes);
          if (bytes) dd.download((uint8_t*)&part[g][at], d_out, bytes);
        });
      });
      g_timer.mark(records_phase);
      for (int g = 0; g < ng && pending_error.empty(); g++) {
        out.write(part[g]);
        pending_error = err[g];
      }
    }
    chain_base += n;
    d.release_all();
    if (!pending_error.empty()) break;
  }
  out.close();
  if (!pending_error.empty()) fail(pending_error);
  return leave(0);
}

/* ---- a chain input: the records (chain.rs:49-55,76-91) and where their data lines are ---------------------------
 * A plain file is split on the device (K23, wga_chain_split): the heads come back, the data lines stay in HBM as the n x 3 array
 * the converters' kernels take, with each chain's first line in d_line_off (the host keeps a copy of those n + 1 offsets: its
 * batches are cut by them).  A file the splitter does not take (CR, non-ASCII bytes, comments, another float syntax for the
 * score, ... : include/wga_hip.h), one of 0xFFFFFFF0 bytes or more, or any file under WGA_CHAIN_READER=host goes through
 * parse_chain: the same records, or the records in front of the reference's error and its text. */
struct ChainInput {
  std::vector<ChainRecord> recs; /* without their `lines`: those are in `lines` or on the device */
  std::string error;             /* the host reader's, "" when the whole file was read */
  bool on_device = false;
  uint64_t* d_lines = nullptr;    /* on_device: 3 u64 per data line, all chains back to back (+ one line of slack), device 0 */
  uint64_t* d_line_off = nullptr; /* on_device: n + 1 */
  std::vector<uint64_t> line_off; /* n + 1 */
  std::vector<uint64_t> lines;    /* host reader, or fetch_lines(): the same array on the host (+ one line of slack) */
  bool have_lines = false;
  /* load_chain(.., keep_on_device = true) with on_device: the text and the heads stay in HBM too (the chain writer, K25, takes
   * them there) and no record is built on the host: recs is empty, the counts are here */
  uint8_t* d_text = nullptr;
  wga_chain_head* d_heads = nullptr;
  uint64_t n_bytes = 0, n_chains = 0, n_data_lines = 0;
  uint64_t n_lines(size_t i) const { return line_off[i + 1] - line_off[i]; }
  /* the device's data lines on the host as well, in one download: for the other devices of --gpus N */
  void fetch_lines(Dev& d) {
    if (have_lines) return;
    lines.assign((size_t)(line_off.back() + 1) * 3, 0);
    if (line_off.back()) d.download(lines.data(), d_lines, (size_t)line_off.back() * 3);
    have_lines = true;
  }
};
/* the splitter's heads as the host's records (without their lines) */
static void chain_records_of_heads(const std::vector<wga_chain_head>& heads, const std::string& text, std::vector<ChainRecord>& recs) {
  recs.reserve(heads.size());
  for (const wga_chain_head& h : heads) {
    ChainRecord r;
    r.score = (double)h.num[0]; /* at most 15 digits: exact */
    r.target_name.assign(text, (size_t)h.tname_off, h.tname_len);
    r.target_size = h.num[1];
    r.target_start = h.num[2];
    r.target_end = h.num[3];
    r.query_name.assign(text, (size_t)h.qname_off, h.qname_len);
    r.query_size = h.num[4];
    r.query_start = h.num[5];
    r.query_end = h.num[6];
    r.chain_id = h.num[7];
    r.target_neg = h.tstrand_neg != 0;
    r.query_neg = h.qstrand_neg != 0;
    recs.push_back(std::move(r));
  }
}
ChainInput load_chain(Dev& d, const std::string* input, bool keep_on_device = false) {
  ChainInput in;
  std::string text = read_all(input);
  /* WGA_CHAIN_READER=host: always the nom-semantics reader (measurements) */
  if (!text.empty() && text.size() < 0xFFFFFFF0ull && !env_is("WGA_CHAIN_READER", "host")) {
    g_timer.mark("file read");
    d.init();
    const size_t n_bytes = text.size();
    text.append(16, '\0'); /* slack behind the text for whole-vector loads */
    uint8_t* d_text = d.upload((const uint8_t*)text.data(), text.size());
    text.resize(n_bytes);
    g_timer.mark("upload");
    uint64_t nc = 0, nd = 0, bad = 0;
    uint32_t status = WGA_CHAIN_FALLBACK;
    d.check(wga_chain_split(d.ctx, d_text, n_bytes, &nc, &nd, &status, &bad, nullptr, 0, nullptr, 0, nullptr));
    if (status == WGA_CHAIN_OK) {
      auto* d_heads = (wga_chain_head*)d.alloc((size_t)(nc + 1) * sizeof(wga_chain_head));
      in.d_lines = (uint64_t*)d.alloc((size_t)(nd + 1) * 3 * sizeof(uint64_t));
      in.d_line_off = (uint64_t*)d.alloc((size_t)(nc + 1) * sizeof(uint64_t));
      d.check(wga_chain_split(d.ctx, d_text, n_bytes, &nc, &nd, &status, &bad, d_heads, nc, in.d_lines, nd, in.d_line_off));
      if (keep_on_device) {
        in.d_text = d_text;
        in.d_heads = d_heads;
        in.n_bytes = n_bytes;
        in.n_chains = nc;
        in.n_data_lines = nd;
        in.on_device = true;
        g_timer.mark("device split");
        return in;
      }
      std::vector<wga_chain_head> heads((size_t)nc);
      in.line_off.resize((size_t)nc + 1);
      if (nc) d.download(heads.data(), d_heads, (size_t)nc);
      d.download(in.line_off.data(), in.d_line_off, (size_t)nc + 1);
      d.release(d_heads);
      d.release(d_text);
      chain_records_of_heads(heads, text, in.recs);
      in.on_device = true;
      g_timer.mark("device split + host records");
      return in;
    }
    d.release(d_text);
  }
  in.recs = parse_chain(text, &in.error);
  in.line_off.assign(1, 0);
  size_t total = 0;
  for (const ChainRecord& r : in.recs) total += r.lines.size();
  in.lines.reserve(total + 3);
  for (ChainRecord& r : in.recs) {
    in.lines.insert(in.lines.end(), r.lines.begin(), r.lines.end());
    in.line_off.push_back(in.lines.size() / 3);
    std::vector<uint64_t>().swap(r.lines);
  }
  in.lines.resize(in.lines.size() + 3);
  in.have_lines = true;
  return in;
}

/* ---- the chain readers' device batch: data lines -> packed ops (wga_chain_lines_ops) -----------------
 * chains [first, first + n) of the input on device d.  in_place: d is the device the splitter ran on, the lines are used where
 * they are (a batch that does not start at chain 0 gets its offsets rebased on the device); otherwise the range's lines are
 * uploaded from the host's array. */
struct ChainBatch {
  wga_cigar_batch cb;
  uint64_t* d_lines = nullptr;
  uint64_t* d_line_off = nullptr;
  uint64_t n_lines = 0;
};
ChainBatch chain_device_batch(Dev& d, const ChainInput& in, size_t first, uint32_t n, bool in_place) {
  ChainBatch b;
  const uint64_t l0 = in.line_off[first];
  b.n_lines = in.line_off[first + n] - l0;
  std::vector<uint8_t> strand(n);
  for (uint32_t k = 0; k < n; k++) strand[k] = in.recs[first + k].query_neg ? 1 : 0;
  if (in_place && in.on_device) {
    b.d_lines = in.d_lines + 3 * l0;
    b.d_line_off = in.d_line_off;
    if (first) {
      b.d_line_off = (uint64_t*)d.alloc(((size_t)n + 1) * 8);
      d.check(wga_chain_line_off_rebase(d.ctx, n, in.d_line_off + first, b.d_line_off));
    }
  } else {
    std::vector<uint64_t> line_off((size_t)n + 1);
    for (uint32_t k = 0; k <= n; k++) line_off[k] = in.line_off[first + k] - l0;
    b.d_lines = d.upload(in.lines.data() + 3 * l0, (size_t)(b.n_lines + 1) * 3); /* what follows the range is its slack */
    b.d_line_off = d.upload(line_off);
  }
  auto* d_cnt = (uint64_t*)d.alloc((size_t)n * 8);
  d.check(wga_chain_lines_ops(d.ctx, n, b.n_lines, b.d_lines, b.d_line_off, d_cnt, nullptr, nullptr));
  uint64_t total = 0;
  uint64_t* d_ooff = d.scan(n, d_cnt, &total);
  auto* d_ops = (uint32_t*)d.alloc((total + 4) * 4);
  d.check(wga_chain_lines_ops(d.ctx, n, b.n_lines, b.d_lines, b.d_line_off, nullptr, d_ops, d_ooff));
  b.cb.d_ops = d_ops;
  b.cb.d_op_off = d_ooff;
  b.cb.d_strand_neg = d.upload(strand);
  b.cb.n_ops = total;
  b.cb.n = n;
  return b;
}

/* ---- chain2maf (converter.rs:268-358) ------------------------------------------------------------------
 * A data line (size, dt, dq) is the op group "size M, dq I, dt D" of parse_chain_to_insert (:360-388), so the
 * rows come from the same kernels as paf2maf.  Records before a failing one are written, like the reference. */
/* the converter's record loop over chains [lo, hi), in resident batches: slices fetched (:309-316: target first, then query, both on
 * the forward strand), data lines -> ops, rows expanded, text handed to the sink (record k of the run is record k of the file).
 * Returns the index of the first failing record, or hi; `err` = the reference's message for it. */
static size_t c2m_run(Dev& d, DevFasta& tf, DevFasta& qf, const ChainInput& in, bool in_place, size_t lo, size_t hi, BatchSink sink,
                      std::string& err) {
  const std::vector<ChainRecord>& recs = in.recs;
  const uint64_t kMaxBytes = 6ull << 30, kMaxLines = 32ull << 20;
  const size_t keep = d.owned.size(); /* the pools stay */
  size_t i0 = lo;
  while (i0 < hi) {
    ExpandJob job;
    uint64_t est = 0, est_lines = 0;
    size_t i = i0;
    std::string fetch_error;
    for (; i < hi; i++) {
      const ChainRecord& r = recs[i];
      if (i > i0 && (est > kMaxBytes || est_lines > kMaxLines)) break;
      uint64_t to, tl, qo, ql;
      try {
        tf.fetch(r.target_name, r.target_start, r.target_end - 1, &to, &tl);
        qf.fetch(r.query_name, r.query_start, r.query_end - 1, &qo, &ql);
      } catch (Error& e) {
        fetch_error = e.msg;
        break;
      }
      job.add(to, tl, qo, ql, 255, r.target_name, r.target_start, r.target_end - r.target_start, r.target_neg,
              r.target_size, r.query_name, r.query_neg ? r.query_size - r.query_end : r.query_start, /* :299-302 */
              r.query_end - r.query_start, r.query_neg, r.query_size);
      est += tl + ql + (tl + ql) / 4;
      est_lines += in.n_lines(i);
    }
    const uint32_t n = (uint32_t)(i - i0);
    if (n) {
      ChainBatch b = chain_device_batch(d, in, i0, n, in_place);
      wga_rec_diag g;
      sink.which = nullptr;
      sink.first = i0;
      sink.records_phase = kChain2mafRecords;
      const uint32_t good = expand_batch(d, b.cb, job, tf.d_pool, tf.bytes, qf.d_pool, qf.bytes, sink, &g);
      d.check(wga_sync(d.ctx));
      if (good < n) {
        if (g.bad_base_pos != WGA_NONE) { /* utils.rs:97, reverse_complement of the query slice (:320-325) */
          char c = qf.at(d, job.q_off[good] + job.q_len[good] - 1 - g.bad_base_pos);
          err = std::string("Invalid Base: `") + c + "`";
        } else {
          err = "panic: String::insert_str beyond the end of the fetched sequence (converter.rs:375,383)";
        }
        d.release_to(keep);
        return i0 + good;
      }
      d.release_to(keep);
    }
    if (!fetch_error.empty()) {
      err = fetch_error;
      return i;
    }
    i0 = i;
  }
  return hi;
}

/* `wgatools --gpus N chain2maf`: the chains in N contiguous ranges, both pools on every device; sizes first (K1 + layout), a
 * prefix gives every record its file offset, rows second, every device pwrite()s its records; the file ends in front of the
 * first failing record. */
static int cmd_chain2maf_multi(Dev& d, ChainInput& in, const std::string& t_fa, const std::string& q_fa, Output& out, int ngpu) {
  const std::vector<ChainRecord>& recs = in.recs;
  std::string pending_error = in.error;
  WorkerDevices wd(d);
  /* device 0 split the file: its worker borrows the reader's context, the others get their ranges' lines */
  std::vector<std::unique_ptr<Dev>>& devs = wd.list(in.on_device);
  if (in.on_device) in.fetch_lines(d);
  std::vector<DevFasta> tf(ngpu), qf(ngpu);
  on_devices(ngpu, [&](int g) {
    devs[g]->init();
    tf[g].load(*devs[g], t_fa);
    qf[g].load(*devs[g], q_fa);
  });
  out.write("#maf version=1.6 convert_from=chain t_seq_path=" + t_fa + " q_seq_path=" + q_fa + "\n");
  uint64_t pos0 = 0;
  const int fd = out.plain_fd(&pos0);
  if (fd < 0) fail("internal error: --gpus needs a plain output file");
  const size_t n = recs.size();
  std::vector<uint64_t> sizes(n, 0), offsets(n + 1, 0);
  std::vector<size_t> bad_at(ngpu, n);
  std::vector<std::string> bad_msg(ngpu);
  auto pass = [&](BatchSink::Mode mode, size_t upto) {
    on_devices(ngpu, [&](int g) {
      const size_t lo = n * (size_t)g / ngpu, hi = std::min(upto, n * (size_t)(g + 1) / ngpu);
      if (lo >= hi) return;
      BatchSink sink;
      sink.mode = mode;
      sink.sizes = &sizes;
      sink.offsets = &offsets;
      sink.fd = fd;
      std::string err;
      const size_t k = c2m_run(*devs[g], tf[g], qf[g], in, g == 0, lo, hi, sink, err);
      if (k < hi && k < bad_at[g]) {
        bad_at[g] = k;
        bad_msg[g] = err;
      }
    });
  };
  pass(BatchSink::SIZES, n);
  size_t first_bad = n;
  for (int g = 0; g < ngpu; g++) first_bad = std::min(first_bad, bad_at[g]);
  offsets[0] = pos0;
  for (size_t i = 0; i < n; i++) offsets[i + 1] = offsets[i] + (i < first_bad ? sizes[i] : 0);
  pass(BatchSink::ROWS, first_bad);
  g_timer.mark(kChain2mafRecords[maf_frame_host_writer() ? 1 : 0]); /* the devices' workers do not mark */
  for (int g = 0; g < ngpu; g++) first_bad = std::min(first_bad, bad_at[g]);
  if (first_bad < n)
    for (int g = 0; g < ngpu; g++)
      if (bad_at[g] == first_bad) pending_error = bad_msg[g];
  if (ftruncate(fd, (off_t)offsets[first_bad]) != 0) fail("IO error:truncate failed");
  out.advance(offsets[first_bad] - pos0);
  out.close();
  if (!pending_error.empty()) fail(pending_error);
  return leave(0);
}

int cmd_chain2maf(const std::string* input, const std::string& t_fa, const std::string& q_fa, Output& out) {
  Dev d;
  ChainInput in = load_chain(d, input);
  const std::vector<ChainRecord>& recs = in.recs;
  std::string pending_error = in.error;
  {
    uint64_t pos = 0;
    if (g_gpus > 1 && recs.size() > 1 && out.plain_fd(&pos) >= 0) return cmd_chain2maf_multi(d, in, t_fa, q_fa, out, g_gpus);
  }
  DevFasta tf, qf;
  d.init();
  tf.load(d, t_fa);
  qf.load(d, q_fa);
  out.write("#maf version=1.6 convert_from=chain t_seq_path=" + t_fa + " q_seq_path=" + q_fa + "\n");
  BatchSink sink;
  sink.out = &out;
  std::string err;
  if (c2m_run(d, tf, qf, in, true, 0, recs.size(), sink, err) < recs.size()) pending_error = err;
  g_timer.mark(kChain2mafRecords[maf_frame_host_writer() ? 1 : 0]); /* a file without a record to write */
  out.close();
  if (!pending_error.empty()) fail(pending_error);
  return leave(0);
}

/* ---- chain2paf (converter.rs:391-416, chain.rs:430-452) ------------------------------------------------
 * GPU: data lines -> ops -> K1 (matches, block length) and the CIGAR text (wga_chain_lines_cigar_text).
 * All records are converted before the first is written (:402-410): an error leaves the output empty. */
/* the PAF rows of chains [lo, hi) of the input on device d, in resident batches; a batch's text goes to `sink` while it is on the device */
static void chain2paf_range(Dev& d, const ChainInput& in, bool in_place, size_t lo, size_t hi,
                            const std::function<void(Dev&, const uint8_t*, size_t)>& sink) {
  const std::vector<ChainRecord>& recs = in.recs;
  d.init();
  const size_t keep = d.owned.size();
  uint64_t kMaxLines = 32ull << 20;
  if (const char* e = getenv("WGA_CHAIN_BATCH_LINES")) kMaxLines = strtoull(e, nullptr, 10); /* the tests reach several batches with small files */
  size_t i0 = lo;
  while (i0 < hi) {
    size_t i = i0;
    uint64_t est = 0;
    for (; i < hi; i++) {
      if (i > i0 && est > kMaxLines) break;
      est += in.n_lines(i);
    }
    d.init();
    const uint32_t n = (uint32_t)(i - i0);
    ChainBatch b = chain_device_batch(d, in, i0, n, in_place);
    auto* d_counts = (wga_cigar_counts*)d.alloc((size_t)n * sizeof(wga_cigar_counts));
    auto* d_diag = (wga_rec_diag*)d.alloc((size_t)n * sizeof(wga_rec_diag));
    d.check(wga_cigar_stat(d.ctx, &b.cb, d_counts, d_diag, nullptr));
    std::vector<wga_cigar_counts> counts(n);
    d.download(counts.data(), d_counts, n);
    auto* d_tb = (uint64_t*)d.alloc((size_t)n * 8);
    d.check(wga_chain_lines_cigar_text(d.ctx, n, b.n_lines, b.d_lines, b.d_line_off, d_tb, nullptr, nullptr));
    std::vector<uint64_t> tb(n);
    d.download(tb.data(), d_tb, n);
    /* record text = host fields up to "cg:Z:" | device CIGAR | "\n" */
    HostFraming f;
    for (uint32_t k = 0; k < n; k++) {
      const ChainRecord& r = recs[i0 + k];
      const wga_cigar_counts& c = counts[k];
      std::string h;
      /* block_length = match + mismatch + del + inv_del (chain.rs:433-435) */
      append_paf_columns(h, r.query_name, r.query_size, r.query_start, r.query_end, r.query_neg, r.target_name, r.target_size,
                         r.target_start, r.target_end, c.match, c.match + c.mismatch + c.del_bp + c.inv_del_bp);
      h += "\tcg:Z:";
      f.add(h, tb[k], "\n");
    }
    auto* d_out = (uint8_t*)d.alloc(f.pos + 64);
    d.check(wga_chain_lines_cigar_text(d.ctx, n, b.n_lines, b.d_lines, b.d_line_off, nullptr, d_out, d.upload(f.mid_off)));
    f.scatter(d, d_out);
    sink(d, d_out, (size_t)f.pos);
    d.release_to(keep);
    i0 = i;
  }
}

/* ---- chain2paf on the device (K27) ------------------------------------------------------------------------------------------
 * A file the chain splitter takes stays in HBM whole (text, heads, data lines, offsets); wga_chain2paf sums, formats and places
 * every record there, and the bytes leave through the pinned-buffer sink (`.gz`: deflated on the device first).  No record is
 * built on the host.  Everything else goes through chain2paf_range: a file the host reader takes, WGA_CHAIN_READER=host,
 * --gpus N > 1, more than 0xFFFFFFF0 chains and data lines, data lines of more than three packed ops each (below),
 * WGA_CHAIN2PAF_WRITER=host (measurements). */
static bool chain2paf_device_wanted() {
  return g_gpus == 1 && !env_is("WGA_CHAIN2PAF_WRITER", "host");
}
/* ... and a file whose data lines need more packed ops than three per line (a value of 2^28 or more is walked in pieces, 2^64 - 1
 * in 2^36 of them): chain2paf_range counts and allocates those ops, and the command keeps what that path does with such a file,
 * the error of an allocation the device cannot make included.  The count is chain_device_batch's first step. */
static bool chain2paf_device_takes(Dev& d, const ChainInput& in) {
  if (!in.on_device || !in.d_text || in.n_chains + in.n_data_lines > 0xFFFFFFF0ull) return false;
  if (in.n_chains == 0) return true;
  const uint32_t n = (uint32_t)in.n_chains;
  auto* d_cnt = (uint64_t*)d.alloc((size_t)n * 8);
  auto* d_ooff = (uint64_t*)d.alloc(((size_t)n + 1) * 8);
  d.check(wga_chain_lines_ops(d.ctx, n, in.n_data_lines, in.d_lines, in.d_line_off, d_cnt, nullptr, nullptr));
  uint64_t n_ops = 0;
  d.scan(n, d_cnt, &n_ops, d_ooff);
  d.release(d_ooff);
  d.release(d_cnt);
  return n_ops <= 3 * in.n_data_lines;
}
/* a file that was kept on the device for a writer that does not take it after all: the host's records and offsets, as
 * load_chain(.., false) leaves them */
static void chain_host_records(Dev& d, ChainInput& in) {
  std::string text((size_t)in.n_bytes, '\0');
  std::vector<wga_chain_head> heads((size_t)in.n_chains);
  in.line_off.resize((size_t)in.n_chains + 1);
  if (in.n_bytes) d.download((uint8_t*)&text[0], in.d_text, (size_t)in.n_bytes);
  if (in.n_chains) d.download(heads.data(), in.d_heads, (size_t)in.n_chains);
  d.download(in.line_off.data(), in.d_line_off, (size_t)in.n_chains + 1);
  chain_records_of_heads(heads, text, in.recs);
}
int chain2paf_path(const std::string* input) { /* `__chain2paf_path` */
  Dev d;
  const bool want = chain2paf_device_wanted();
  ChainInput in = load_chain(d, input, want);
  printf("%s\n", want && chain2paf_device_takes(d, in) ? "device" : "host");
  return 0;
}

int cmd_chain2paf(const std::string* input, Output& out) {
  Dev d;
  const bool want = chain2paf_device_wanted();
  ChainInput in = load_chain(d, input, want);
  if (want && chain2paf_device_takes(d, in)) { /* all records are made before the first byte is written, like the host path */
    if (in.n_chains) {
      const DevText t = two_call_text(
          d, (size_t)wga_chain2paf_work_bytes(in.n_chains, in.n_data_lines) + 16,
          [&](void* d_work, uint64_t* bytes, uint8_t* d_out) {
            return wga_chain2paf(d.ctx, in.d_text, in.n_bytes, in.d_heads, in.n_chains, in.d_lines, in.d_line_off, d_work, bytes, d_out);
          },
          true);
      d.check(wga_sync(d.ctx));
      g_timer.mark("chain2paf records (device)");
      stream_out(d, out, t.d_out, t.bytes, false);
      g_timer.mark("copy out + write");
    }
    out.close();
    return leave(0);
  }
  if (in.on_device && in.d_text) chain_host_records(d, in);
  const std::vector<ChainRecord>& recs = in.recs;
  if (!in.error.empty()) {
    out.close();
    fail(in.error);
  }
  if (g_gpus == 1 || recs.size() < 2) {
    if (!recs.empty())
      chain2paf_range(d, in, true, 0, recs.size(), [&](Dev& dg, const uint8_t* d_out, size_t bytes) {
        dg.check(wga_sync(dg.ctx));
        g_timer.mark("chain2paf records (host)");
        stream_out(dg, out, d_out, bytes, false);
        g_timer.mark("copy out + write");
      });
  } else { /* --gpus N: the chains in contiguous ranges over the devices, the rows meet in input order */
    const int ng = g_gpus;
    const size_t n = recs.size();
    WorkerDevices wd(d);
    /* device 0 split the file: its worker borrows the reader's context, the others get their ranges' lines */
    std::vector<std::unique_ptr<Dev>>& devs = wd.list(in.on_device);
    if (in.on_device) in.fetch_lines(d);
    std::vector<std::string> part(ng);
    on_devices(ng, [&](int g) {
      const size_t lo = n * (size_t)g / ng, hi = n * (size_t)(g + 1) / ng;
      if (lo == hi) return;
      chain2paf_range(*devs[g], in, g == 0, lo, hi, [&](Dev& dd, const uint8_t* d_out, size_t bytes) {
        const size_t at = part[g].size();
        part[g].resize(at + bytes);
        if (bytes) dd.download((uint8_t*)&part[g][at], d_out, bytes);
      });
    });
    g_timer.mark("chain2paf records (host)");
    for (const std::string& t : part) out.write(t);
  }
  out.close();
  return leave(0);
}

/* ---- maf2chain (converter.rs:57-91) ---------------------------------------------------------------------
 * GPU: K3 column-pair runs -> packed ops (wga_maf_runs_ops) -> data lines and trims (wga_cigar_chain; '=' and X
 * runs add up into one block like cigar_cat's M) -> chain headers (chain.rs:103-140,185-203), record ends and the layout
 * (wga_chain_heads, K30).  Host: one wga_maf2paf_head per block, as maf2paf fills it; the names are read where the rows were
 * uploaded (p.names_in_rows) or gathered.  Only the text's length comes back (K3's runs hold no op K10 rejects: every block is
 * good).  WGA_CHAIN_HEAD_WRITER=host: the headers printed by one host thread from the downloaded trims, as before K30. */
/* the chains of blocks recs[0 .. n), whose rows stand on device d (p); chain ids from chain_id0.  The text stays on the device:
 * *d_text, *bytes. */
static void maf2chain_text(Dev& d, const MafRows& p, const MafRecord* const* recs, uint32_t n, uint64_t chain_id0,
                           const uint8_t** d_text, uint64_t* bytes) {
  const wga_cigar_batch cb = maf_runs_batch(d, p, n, maf_runs(d, p, n));
  const ChainTrims t = chain_trims(d, cb);
  if (!chain_head_host_writer()) {
    RecordHeads hd(n, &p);
    for (uint32_t k = 0; k < n; k++) hd.add(*recs[k]);
    hd.upload(d);
    uint32_t good = 0;
    *d_text = chain_text_device(d, cb, hd, t, chain_id0, bytes, &good);
    return;
  }
  std::vector<wga_chain_trim_t> trim(n);
  std::vector<uint64_t> nb(n);
  d.download(trim.data(), t.d_trim, n);
  d.download(nb.data(), t.d_nb, n);
  HostFraming f;
  for (uint32_t k = 0; k < n; k++) {
    const MafRecord& r = *recs[k];
    std::string h;
    append_chain_head(h, r.t().name, r.t().size, r.t().start, r.t().start + r.t().align_size, r.q().name, r.q().size, r.q().neg,
                      r.query_start(), r.query_end(), trim[k], chain_id0 + (uint64_t)k);
    f.add(h, nb[k], "\n\n");
  }
  *d_text = chain_text_host(d, cb, f);
  *bytes = f.pos;
}

int cmd_maf2chain(const std::string* input, const std::string* query_name, Output& out) {
  Dev d;
  MafDevices md(d);
  MafChunks chunks(input);
  MafInput min;
  uint64_t chain_base = 0; /* chain id = index of the block in the whole input */
  const char* const records_phase = chain_head_host_writer() ? "maf2chain records (host)" : "maf2chain records (device)";
  std::string pending_error;
  while (pending_error.empty() && chunks.next(d, min)) {
  std::vector<MafRecord>& recs = min.recs;
  const uint64_t n_in_piece = recs.size();
  /* set_query_idx_byname fails per record, after the earlier records were written (:66-73) */
  size_t n_ok = recs.size();
  for (size_t k = 0; k < recs.size() && pending_error.empty(); k++) {
    MafRecord& r = recs[k];
    if (query_name) {
      size_t x = 0;
      for (; x < r.slines.size(); x++)
        if (r.slines[x].name == *query_name) break;
      if (x == r.slines.size()) {
        pending_error = "Query name:" + *query_name + " not found in MAF";
        n_ok = k;
        break;
      }
      r.query_idx = x;
    }
    if (r.query_idx >= r.slines.size()) {
      pending_error = "panic: MAF block with a single s-line has no query row (maf.rs:426 index out of bounds)";
      n_ok = k;
    }
  }
  recs.resize(n_ok);
  if (!recs.empty()) {
    const std::vector<const MafRecord*> all = all_records(recs);
    if (md.count() == 1) {
      md.run(min, all, false, [&](int, Dev& dg, const MafRows& p, uint32_t lo, uint32_t cnt) {
        const uint8_t* d_text = nullptr;
        uint64_t bytes = 0;
        maf2chain_text(dg, p, all.data() + lo, cnt, chain_base + lo, &d_text, &bytes);
        dg.check(wga_sync(dg.ctx));
        g_timer.mark(records_phase);
        stream_out(dg, out, d_text, (size_t)bytes);
      });
    } else { /* --gpus N: a piece's blocks in contiguous ranges over the devices, the chains meet in block order */
      std::vector<std::string> part(md.count());
      md.run(min, all, false, [&](int g, Dev& dg, const MafRows& p, uint32_t lo, uint32_t cnt) {
        const uint8_t* d_text = nullptr;
        uint64_t bytes = 0;
        maf2chain_text(dg, p, all.data() + lo, cnt, chain_base + lo, &d_text, &bytes);
        part[g].resize((size_t)bytes);
        if (bytes) dg.download((uint8_t*)&part[g][0], d_text, bytes);
      });
      g_timer.mark(records_phase);
      for (const std::string& t : part) out.write(t);
    }
  }
  chain_base += n_in_piece;
  md.release_all();
  }
  out.close();
  if (!pending_error.empty()) fail(pending_error);
  return leave(0);
}
