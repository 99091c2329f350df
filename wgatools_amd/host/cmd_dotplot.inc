/* cmd_dotplot.inc — part of wgatools_main.cpp (included there, inside its namespace: the commands share the device helpers, readers and
 * writers defined in front of the include). */
/* ---- dotplot --out-format csv (tools/dotplot.rs; SURVEY.md 8f rank 4) -----------------------------------
 * base-level: segments from wga_cigar_dotplot (PAF: device tokeniser; MAF: K3 runs -> wga_maf_runs_ops), their rows
 * written on the device (K26) unless WGA_DOTPLOT_WRITER=host;
 * overview: one row per record, identity = matched / target_align_size from K1 / K3, written on the device (K34,
 * wga_dotplot_overview) where the counters lie unless WGA_DOTPLOT_WRITER=host: only K1's diagnostics and the text come back.
 * With -d on PAF nothing is tokenised and K34 writes "1.0"; with -d on MAF no device holds anything of the blocks, and the rows
 * stay the host's loop (an upload of the names would be all the device got).  All data is generated
 * before anything is written (:208-262), so an error leaves the output empty.  The html / json outputs embed
 * the reference's Vega-Lite document and are not provided. */
/* the records of one device's share of a piece, as the csv rows need them */
struct DotRecs {
  std::vector<std::string> t_names, q_names;
  std::vector<uint64_t> ts, te, qs, qe, ali;
  std::vector<uint8_t> negs;
  void add(const std::string& t, const std::string& q, uint64_t ts_, uint64_t te_, uint64_t qs_, uint64_t qe_, bool neg, uint64_t a) {
    t_names.push_back(t);
    q_names.push_back(q);
    ts.push_back(ts_);
    te.push_back(te_);
    qs.push_back(qs_);
    qe.push_back(qe_);
    negs.push_back(neg ? 1 : 0);
    ali.push_back(a);
  }
};
/* WGA_DOTPLOT_WRITER=host: the rows are printed on the host from the downloaded segments / counters (measurements, and the
 * cross-check of the device writers: same bytes) */
static bool dotplot_host_writer() { return env_is("WGA_DOTPLOT_WRITER", "host"); }
/* csv rows (no header line) of the records R: base-level segments from wga_cigar_dotplot over the device batch cb, written as
 * text on the device (K26, wga_dotplot_csv), or one overview row per record from the counts */
static std::string dotplot_rows(Dev& d, bool base, bool no_identity, uint64_t cutoff, const DotRecs& R, const wga_cigar_batch& cb,
                                const std::vector<wga_cigar_counts>& counts) {
  std::string text;
  const uint32_t n = (uint32_t)R.t_names.size();
  if (base) {
    if (n) {
      auto* d_cnt = (uint64_t*)d.alloc((size_t)n * 8);
      auto *d_ts = d.upload(R.ts), *d_qs = d.upload(R.qs);
      d.check(wga_cigar_dotplot(d.ctx, &cb, cutoff, d_ts, d_qs, d_cnt, nullptr, nullptr));
      uint64_t n_rows = 0;
      uint64_t* d_off = d.scan(n, d_cnt, &n_rows);
      auto* d_segs = (uint64_t*)d.alloc((n_rows + 1) * 5 * 8);
      d.check(wga_cigar_dotplot(d.ctx, &cb, cutoff, d_ts, d_qs, nullptr, d_segs, d_off));
      /* every row ends in its record's tail: the names quoted once per record, the newline */
      std::string tails;
      std::vector<uint64_t> tail_off(n + 1);
      for (uint32_t k = 0; k < n; k++) {
        tail_off[k] = tails.size();
        tails.push_back(',');
        append_csv_field(tails, R.t_names[k], ',');
        tails.push_back(',');
        append_csv_field(tails, R.q_names[k], ',');
        tails.push_back('\n');
      }
      tail_off[n] = tails.size();
      if (!dotplot_host_writer() && n_rows <= 0xFFFFFFF0ull) {
        /* K26: the rows are written where the segments are and come back as text */
        auto* d_tails = d.upload((const uint8_t*)tails.data(), tails.size());
        auto* d_tail_off = d.upload(tail_off);
        const DevText t = two_call_text(d, (size_t)wga_dotplot_csv_work_bytes(n_rows) + 16, [&](void* d_work, uint64_t* bytes, uint8_t* d_out) {
          return wga_dotplot_csv(d.ctx, n, d_segs, d_off, d_tails, d_tail_off, d_work, bytes, d_out);
        });
        text.resize(t.bytes);
        if (t.bytes) d.download((uint8_t*)&text[0], t.d_out, t.bytes);
      } else {
        std::vector<uint64_t> off(n + 1);
        d.download(off.data(), d_off, n + 1);
        std::vector<uint64_t> segs(n_rows * 5);
        if (n_rows) d.download(segs.data(), d_segs, n_rows * 5);
        for (uint32_t k = 0; k < n; k++) {
          for (uint64_t x = off[k]; x < off[k + 1]; x++) {
            const uint64_t* sg = &segs[5 * x];
            for (int f = 0; f < 4; f++) {
              append_u64(text, sg[f]);
              text.push_back(',');
            }
            text.push_back("MID"[sg[4]]);
            text.append(tails, tail_off[k], tail_off[k + 1] - tail_off[k]);
          }
        }
      }
    }
  } else {
    for (uint32_t k = 0; k < n; k++) {
      const uint64_t a[] = {R.ts[k], R.te[k], R.negs[k] ? R.qe[k] : R.qs[k], R.negs[k] ? R.qs[k] : R.qe[k]}; /* dotplot.rs:400-406 */
      for (uint64_t v : a) {
        append_u64(text, v);
        text.push_back(',');
      }
      text += format_f64(no_identity ? 1.0 : (double)counts[k].match / (double)R.ali[k]);
      text.push_back(',');
      append_csv_field(text, R.t_names[k], ',');
      text.push_back(',');
      append_csv_field(text, R.q_names[k], ',');
      text.push_back('\n');
    }
  }
  return text;
}
/* ---- overview on the device (K34) ---------------------------------------------------------------------------------------------
 * the heads wga_dotplot_overview takes: a record's four numbers as printed, the divisor and where its two names stand */
struct DotOvHeads : NameSpans {
  std::vector<wga_dotplot_ov_head> heads;
  explicit DotOvHeads(uint32_t n, const MafRows* p = nullptr) : NameSpans(p) { heads.reserve(n); }
  void add(const std::string& t_name, uint64_t t_at, const std::string& q_name, uint64_t q_at, uint64_t ts, uint64_t te, uint64_t qs,
           uint64_t qe, bool neg, uint64_t ali) {
    wga_dotplot_ov_head h;
    h.ref_start = ts, h.ref_end = te;
    h.q_first = neg ? qe : qs, h.q_second = neg ? qs : qe; /* dotplot.rs:400-406 */
    h.align_size = ali;
    span(t_name, t_at, h.rname_off, h.rname_len);
    span(q_name, q_at, h.qname_off, h.qname_len);
    heads.push_back(h);
  }
};
/* a range's rows can be K34's */
static bool dotplot_overview_on_device(size_t n) { return !dotplot_host_writer() && n <= 0xFFFFFFF0ull; }
/* the rows of the records of hd, whose counters stand on d (nullptr: no_identity), as text */
static std::string dotplot_overview_rows(Dev& d, DotOvHeads& hd, const wga_cigar_counts* d_counts) {
  std::string text;
  const uint32_t n = (uint32_t)hd.heads.size();
  if (n == 0) return text;
  record_rows_text(d, hd, hd.heads, (size_t)wga_dotplot_overview_work_bytes(n), text,
                   [&](const wga_dotplot_ov_head* d_heads, void* d_work, uint64_t* d_row_off, uint64_t* total, uint8_t* d_out) {
                     return wga_dotplot_overview(d.ctx, n, hd.d_names, hd.n_name_bytes, d_heads, d_counts, d_counts ? 0 : 1, d_work,
                                                 d_row_off, total, d_out);
                   });
  return text;
}
/* records [lo, hi) of a PAF piece: the counters stay where K1 left them, only the diagnostics come back; the names are read in
 * the uploaded piece where the device reader took it */
static std::string dotplot_paf_overview(Dev& d, const PafInput& pin, size_t lo, size_t hi, const uint8_t* d_text_here, bool no_identity,
                                        std::string& err) {
  const uint32_t n = (uint32_t)(hi - lo);
  if (n == 0) return std::string();
  d.init();
  const wga_cigar_counts* d_counts = nullptr;
  if (!no_identity) {
    CigarTexts cigars;
    wga_cigar_batch cb;
    err = device_tokenise(d, pin, lo, n, cigars, &cb, nullptr, nullptr, d_text_here);
    if (cb.n) { /* get_stat (paf.rs:205-209): ops outside M = X I D are an error */
      auto* d_cnt = (wga_cigar_counts*)d.alloc((size_t)cb.n * sizeof(wga_cigar_counts));
      auto* d_diag = (wga_rec_diag*)d.alloc((size_t)cb.n * sizeof(wga_rec_diag));
      d.check(wga_cigar_stat(d.ctx, &cb, d_cnt, d_diag, nullptr));
      std::vector<wga_rec_diag> diag(cb.n);
      d.download(diag.data(), d_diag, cb.n);
      for (uint32_t k = 0; k < cb.n; k++)
        if (diag[k].bad_op_idx != WGA_NONE) {
          err = bad_op_message(cigars, k, diag[k]);
          break;
        }
      d_counts = d_cnt;
    }
    if (!err.empty() || cb.n != n) return std::string();
  }
  MafRows in_piece;
  in_piece.d_rows = d_text_here ? d_text_here : pin.d_text;
  in_piece.names_in_rows = pin.on_device;
  in_piece.n_row_bytes = pin.text.size();
  DotOvHeads hd(n, &in_piece);
  for (size_t k = lo; k < hi; k++) {
    const PafRecord& r = pin.recs[k];
    hd.add(r.target_name, r.tname_off, r.query_name, r.qname_off, r.target_start, r.target_end, r.query_start, r.query_end, r.neg,
           r.target_end - r.target_start);
  }
  return dotplot_overview_rows(d, hd, d_counts);
}
/* blocks recs[0 .. n) of a MAF piece, whose rows stand on device d (p): the counters stay where K3 left them */
static std::string dotplot_maf_overview(Dev& d, const MafRows& p, const MafRecord* const* recs, uint32_t n) {
  if (n == 0) return std::string();
  const MafRuns runs = maf_runs(d, p, n, true);
  DotOvHeads hd(n, &p);
  for (uint32_t k = 0; k < n; k++) {
    const MafRecord& r = *recs[k];
    hd.add(r.t().name, r.t().name_off, r.q().name, r.q().name_off, r.t().start, r.t().start + r.t().align_size, r.query_start(),
           r.query_end(), r.q().neg, r.t().align_size);
  }
  return dotplot_overview_rows(d, hd, runs.d_counts);
}

/* records [lo, hi) of a PAF piece on device d; `err` = the reference's message for the first failing record of the range */
static std::string dotplot_paf_part(Dev& d, const PafInput& pin, size_t lo, size_t hi, const uint8_t* d_text_here, bool base,
                                    bool no_identity, uint64_t cutoff, std::string& err) {
  if (!base && dotplot_overview_on_device(hi - lo)) return dotplot_paf_overview(d, pin, lo, hi, d_text_here, no_identity, err);
  DotRecs R;
  for (size_t k = lo; k < hi; k++) {
    const PafRecord& r = pin.recs[k];
    R.add(r.target_name, r.query_name, r.target_start, r.target_end, r.query_start, r.query_end, r.neg, r.target_end - r.target_start);
  }
  wga_cigar_batch cb;
  cb.n = 0;
  std::vector<wga_cigar_counts> counts;
  const uint32_t n = (uint32_t)(hi - lo);
  if (n && (base || !no_identity)) {
    d.init();
    CigarTexts cigars;
    err = device_tokenise(d, pin, lo, n, cigars, &cb, nullptr, nullptr, d_text_here);
    if (!base && cb.n) { /* get_stat (paf.rs:205-209): ops outside M = X I D are an error */
      auto* d_counts = (wga_cigar_counts*)d.alloc((size_t)cb.n * sizeof(wga_cigar_counts));
      auto* d_diag = (wga_rec_diag*)d.alloc((size_t)cb.n * sizeof(wga_rec_diag));
      d.check(wga_cigar_stat(d.ctx, &cb, d_counts, d_diag, nullptr));
      counts.resize(cb.n);
      std::vector<wga_rec_diag> diag(cb.n);
      d.download(counts.data(), d_counts, cb.n);
      d.download(diag.data(), d_diag, cb.n);
      for (uint32_t k = 0; k < cb.n; k++)
        if (diag[k].bad_op_idx != WGA_NONE) {
          err = bad_op_message(cigars, k, diag[k]);
          break;
        }
    }
    if (!err.empty()) return std::string();
  }
  return dotplot_rows(d, base, no_identity, cutoff, R, cb, counts);
}
/* blocks recs[0 .. n) of a MAF piece, whose rows stand on device d (p) */
static std::string dotplot_maf_part(Dev& d, const MafRows& p, const MafRecord* const* recs, uint32_t n, bool base, bool no_identity,
                                    uint64_t cutoff) {
  if (!base && !no_identity && dotplot_overview_on_device(n)) return dotplot_maf_overview(d, p, recs, n);
  DotRecs R;
  for (uint32_t k = 0; k < n; k++) {
    const MafRecord& r = *recs[k];
    R.add(r.t().name, r.q().name, r.t().start, r.t().start + r.t().align_size, r.query_start(), r.query_end(), r.q().neg,
          r.t().align_size);
  }
  wga_cigar_batch cb;
  cb.n = 0;
  std::vector<wga_cigar_counts> counts;
  if (n && (base || !no_identity)) {
    const MafRuns r = maf_runs(d, p, n, !base); /* the overview wants the counts only */
    if (!base) {
      counts.resize(n);
      d.download(counts.data(), r.d_counts, n);
    } else {
      cb = maf_runs_batch(d, p, n, r);
    }
  }
  return dotplot_rows(d, base, no_identity, cutoff, R, cb, counts);
}

int cmd_dotplot(const std::string* input, const std::string& format, const std::string& out_format,
                const std::string& mode, bool no_identity, uint64_t cutoff, const std::string* query_name, Output& out) {
  if (mode != "base-level" && mode != "overview") fail("invalid value '" + mode + "' for '--mode <MODE>'");
  if (out_format != "csv") {
    if (out_format == "html" || out_format == "json")
      fail("out-format `" + out_format + "` embeds the reference's Vega-Lite document and is not provided by this engine (use --out-format csv)");
    fail("invalid value '" + out_format + "' for '--out-format <OUT_FORMAT>'");
  }
  if (format != "maf" && format != "paf") fail("Only support MAF and PAF format");
  const bool base = mode == "base-level";
  /* WGA_TIMING=1 names the writer of the rows; the overview rows of a MAF under -d are always the host's */
  const bool device_rows = !dotplot_host_writer() && (base || format == "paf" || !no_identity);
  const char* const rows_phase = device_rows ? "dotplot rows (device)" : "dotplot rows (host)";
  std::string text; /* all data is generated before anything is written (dotplot.rs:208-262) */
  uint64_t n_records = 0;
  Dev d;
  /* --gpus N: a piece's records / blocks in contiguous ranges over the devices; the rows meet in input order */
  if (format == "paf") {
    PafChunks chunks(input, false);
    PafInput pin;
    WorkerDevices wd(d);
    while (chunks.next(d, pin)) {
      const size_t n = pin.recs.size();
      n_records += n;
      const int ng = g_gpus;
      std::vector<std::string> part(ng), err(ng);
      if (ng == 1) {
        part[0] = dotplot_paf_part(d, pin, 0, n, nullptr, base, no_identity, cutoff, err[0]);
      } else {
        wd.run(pin, [&](int g, Dev& dg, size_t lo, size_t hi, const uint8_t* d_text) {
          part[g] = dotplot_paf_part(dg, pin, lo, hi, d_text, base, no_identity, cutoff, err[g]);
        });
      }
      for (int g = 0; g < ng; g++) {
        if (!err[g].empty()) {
          out.close();
          fail(err[g]);
        }
        text += part[g];
      }
      g_timer.mark(rows_phase);
      d.release_all();
    }
  } else {
    MafDevices md(d);
    MafChunks chunks(input);
    MafInput min;
    while (chunks.next(d, min)) {
      std::vector<MafRecord>& recs = min.recs;
      select_query(recs, query_name);
      n_records += recs.size();
      if (!recs.empty()) {
        const std::vector<const MafRecord*> all = all_records(recs);
        std::vector<std::string> part(md.count());
        if (base || !no_identity) {
          md.run(min, all, false, [&](int g, Dev& dg, const MafRows& p, uint32_t lo, uint32_t cnt) {
            part[g] = dotplot_maf_part(dg, p, all.data() + lo, cnt, base, no_identity, cutoff);
          });
        } else {
          part[0] = dotplot_maf_part(d, MafRows(), all.data(), (uint32_t)all.size(), base, no_identity, cutoff);
        }
        for (const std::string& t : part) text += t;
      }
      g_timer.mark(rows_phase);
      md.release_all();
    }
  }
  g_timer.mark(rows_phase);
  /* the header line: base-level once a segment exists, overview once a record does */
  if (base ? !text.empty() : n_records != 0)
    text = std::string(base ? "ref_start,ref_end,query_start,query_end,cigar,ref_chro,query_chro\n"
                            : "ref_start,ref_end,query_start,query_end,identity,ref_chro,query_chro\n") + text;
  out.write(text);
  out.close();
  return leave(0);
}
