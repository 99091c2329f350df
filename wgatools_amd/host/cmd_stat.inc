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
          bad_msg[g] = bad_op_message(cigars, k, diag[k]);
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

/* `stat -e` with the device writer (K33): per piece the counters stay on device 0 where K1 left them (--gpus N: they meet on the
 * host as for the merged table and are uploaded there), the host fills one head per record, and the piece's rows come back as
 * text (StatRows, cmd_common.inc).  Buffered driver: nothing is written before the last piece's records are counted. */
/* Without -e the same loop feeds the merged table (K36, StatTable): the piece's pairs come back instead of its rows. */
static int stat_paf_rows_device(const std::string* input, bool each, Output& out) {
  Dev d;
  PafChunks chunks(input, false);
  PafInput pin;
  WorkerDevices wd(d); /* --gpus N */
  StatRows rows;
  StatTable table;
  while (chunks.next(d, pin)) {
    const std::vector<PafRecord>& recs = pin.recs;
    const uint32_t n = (uint32_t)recs.size();
    d.init();
    const wga_cigar_counts* d_counts = nullptr;
    if (g_gpus > 1) {
      std::vector<wga_cigar_counts> counts(n);
      stat_piece_multi(wd.list(), pin, counts);
      d_counts = d.upload(counts);
    } else {
      std::vector<wga_cigar_counts> none;
      std::string op_err;
      const std::string e = paf_counts(d, pin, n, none, op_err, &d_counts);
      if (!op_err.empty()) fail(op_err);
      if (!e.empty()) fail(e);
    }
    MafRows in_piece; /* the names are read in the uploaded piece where the device reader took it */
    in_piece.d_rows = pin.d_text;
    in_piece.names_in_rows = pin.on_device;
    in_piece.n_row_bytes = pin.text.size();
    StatRowHeads hd(n, &in_piece);
    for (const PafRecord& r : recs) {
      if (each) rows.note(r.target_name);
      hd.add(r.target_name, r.tname_off, r.target_length, r.target_start, r.query_name, r.qname_off, r.query_length, r.query_start);
    }
    if (each) rows.piece(d, hd, d_counts);
    else table.piece(d, hd, d_counts, [&](size_t k) { return std::make_pair(&recs[k].target_name, &recs[k].query_name); });
    d.release_all();
  }
  if (each) rows.write(out);
  else table.write(d, out);
  out.close();
  return leave(0);
}

int cmd_stat_paf(const std::string* input, bool each, Output& out) {
  if (!stat_host_writer()) return stat_paf_rows_device(input, each, out);
  Dev d;
  PafChunks chunks(input, false);
  std::vector<StatInput> in;
  PafInput pin;
  WorkerDevices wd(d); /* --gpus N */
  while (chunks.next(d, pin)) { /* one piece of the file at a time; only the per-record statistics are kept */
    const std::vector<PafRecord>& recs = pin.recs;
    const uint32_t n = (uint32_t)recs.size();
    std::vector<wga_cigar_counts> counts(n);
    d.init();
    if (g_gpus > 1) {
      stat_piece_multi(wd.list(), pin, counts);
    } else { /* buffered driver: nothing is written on error; an op K1 rejects speaks before a later record's tag or tokeniser error */
      std::string op_err;
      const std::string e = paf_counts(d, pin, n, counts, op_err);
      if (!op_err.empty()) fail(op_err);
      if (!e.empty()) fail(e);
    }
    in.reserve(in.size() + n);
    for (uint32_t k = 0; k < n; k++) {
      const PafRecord& r = recs[k];
      in.push_back(StatInput{r.target_name, r.query_name, r.target_length, r.query_length, r.target_start,
                             r.query_start, recstat_from(counts[k])});
    }
    d.release_all();
  }
  out.write(stat_tsv(in, each));
  g_timer.mark(each ? "stat rows (host)" : "stat table (host)");
  out.close();
  return leave(0);
}

/* `stat -e` on MAF with the device writer: as stat_paf_rows_device, over K3's counters.  One device: they stay where K3 left them
 * and the names are read in the uploaded piece; --gpus N: they arrive on the host and are uploaded to device 0 with the names. */
static int stat_maf_rows_device(const std::string* input, bool each, const std::string* query_name, Output& out) {
  Dev d;
  MafDevices md(d);
  MafChunks chunks(input);
  MafInput min;
  StatRows rows;
  StatTable table;
  while (chunks.next(d, min)) {
    std::vector<MafRecord>& recs = min.recs;
    select_query(recs, query_name);
    const uint32_t n = (uint32_t)recs.size();
    if (n) {
      if (each)
        for (const MafRecord& r : recs) rows.note(r.t().name);
      auto piece = [&](Dev& dg, StatRowHeads& hd, const wga_cigar_counts* d_counts) {
        if (each) rows.piece(dg, hd, d_counts);
        else table.piece(dg, hd, d_counts, [&](size_t k) { return std::make_pair(&recs[k].t().name, &recs[k].q().name); });
      };
      auto heads = [&](StatRowHeads& hd) {
        for (const MafRecord& r : recs)
          hd.add(r.t().name, r.t().name_off, r.t().size, r.t().start, r.q().name, r.q().name_off, r.q().size, r.query_start());
      };
      std::vector<wga_cigar_counts> counts(md.count() > 1 ? n : 0);
      md.run(min, all_records(recs), false, [&](int, Dev& dg, const MafRows& p, uint32_t lo, uint32_t cnt) {
        const MafRuns R = maf_runs(dg, p, cnt, true);
        if (md.count() > 1) {
          dg.download(counts.data() + lo, R.d_counts, cnt);
          return;
        }
        StatRowHeads hd(n, &p);
        heads(hd);
        piece(dg, hd, R.d_counts);
      });
      if (md.count() > 1) {
        d.init();
        StatRowHeads hd(n);
        heads(hd);
        piece(d, hd, d.upload(counts));
      }
    }
    md.release_all();
  }
  if (each) rows.write(out);
  else table.write(d, out);
  out.close();
  return leave(0);
}

int cmd_stat_maf(const std::string* input, bool each, const std::string* query_name, Output& out) {
  if (!stat_host_writer()) return stat_maf_rows_device(input, each, query_name, out);
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
  g_timer.mark(each ? "stat rows (host)" : "stat table (host)");
  out.close();
  return leave(0);
}
