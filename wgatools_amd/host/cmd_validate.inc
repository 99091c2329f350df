/* cmd_validate.inc — part of wgatools_main.cpp (included there, inside its namespace: the commands share the device helpers, readers and
 * writers defined in front of the include). */
/* ---- validate --fix on the device (K29) ----------------------------------------------------------------------------------------
 * `--fix` changes at most two numbers of a record, and for a plain line in canonical decimal the csv writer gives back every other
 * byte as it stands (K24's observation).  So a piece wga_paf_fix_plan takes stays where it was uploaded: split (K13), the cg:Z:
 * spans (plan), tokeniser (K8), counts (K1), and wga_paf_fix writes the piece's rows and its share of the two invalid lists there.
 * Only the sizes, the two lists and the rows come back — and the tokeniser's and K1's per-record diagnostics, 40 bytes a record:
 * if they report anything the piece is the host path's, which words the reference's error.  No record is built and no line table
 * is downloaded.  Any other piece goes through parse_paf and cmd_validate's loop with the running record, line and byte counters, so
 * device and host pieces may alternate within one file.  WGA_VALIDATE_WRITER=host or WGA_PAF_READER=host: every piece on the host. */
struct ValidateAcc {
  uint64_t n_total = 0, q_bad = 0, t_bad = 0;
  std::string q_list, t_list, rows;
};
static bool validate_fix_host_forced() {
  return env_is("WGA_VALIDATE_WRITER", "host") || env_is("WGA_PAF_READER", "host");
}
/* one piece on the device.  False, with nothing left on the device and `acc` as it was: the piece is the host path's. */
static bool validate_fix_device(Dev& d, std::string& text, ValidateAcc& acc) {
  if (validate_fix_host_forced() || text.empty() || text.size() >= 0xFFFFFFF0ull) return false;
  d.init();
  const size_t owned0 = d.owned.size();
  const uint64_t n_bytes = text.size();
  text.append(16, '\0'); /* slack behind the text for whole-vector loads */
  auto* d_text = d.upload((const uint8_t*)text.data(), text.size());
  text.resize(text.size() - 16);
  g_timer.mark("upload");
  uint64_t n_lines = 0, n_rec = 0, untaken = WGA_NONE;
  d.check(wga_paf_split(d.ctx, d_text, n_bytes, &n_lines, nullptr, 0));
  auto* d_lines = (wga_paf_line*)d.alloc((size_t)(n_lines + 1) * sizeof(wga_paf_line));
  d.check(wga_paf_split(d.ctx, d_text, n_bytes, &n_lines, d_lines, n_lines));
  void* d_work = d.alloc((size_t)wga_paf_fix_work_bytes(n_lines));
  d.check(wga_paf_fix_plan(d.ctx, d_text, n_bytes, d_lines, n_lines, d_work, &n_rec, &untaken, nullptr, nullptr));
  g_timer.mark("device split + plan");
  auto leave_to_host = [&]() {
    d.release_to(owned0);
    return false;
  };
  if (untaken != WGA_NONE || n_rec > 0xFFFFFFF0ull) return leave_to_host();
  if (n_rec == 0) { /* comments and blank lines only */
    d.release_to(owned0);
    return true;
  }
  const uint32_t n = (uint32_t)n_rec;
  auto* d_beg = (uint64_t*)d.alloc(((size_t)n + 1) * 8);
  auto* d_end = (uint64_t*)d.alloc(((size_t)n + 1) * 8);
  d.check(wga_paf_fix_plan(d.ctx, d_text, n_bytes, d_lines, n_lines, d_work, &n_rec, &untaken, d_beg, d_end));
  auto* d_cnt = (uint64_t*)d.alloc((size_t)n * 8);
  auto* d_err = (wga_tok_err*)d.alloc((size_t)n * sizeof(wga_tok_err));
  d.check(wga_cigar_tokenise_spans(d.ctx, n, d_text, d_beg, d_end, d_cnt, d_err, nullptr, nullptr));
  uint64_t n_ops = 0;
  uint64_t* d_ooff = d.scan(n, d_cnt, &n_ops);
  auto* d_ops = (uint32_t*)d.alloc((size_t)(n_ops + 4) * 4);
  d.check(wga_cigar_tokenise_spans(d.ctx, n, d_text, d_beg, d_end, d_cnt, d_err, d_ops, d_ooff));
  std::vector<wga_tok_err> errs(n);
  d.download(errs.data(), d_err, n);
  for (const wga_tok_err& e : errs)
    if (e.err) return leave_to_host();
  /* both ends add a strand's slot and its inv_* twin (validate.rs:82-100), so the sums do not ask for the strands: all `+` */
  auto* d_strand = (uint8_t*)d.alloc((size_t)n + 16);
  d.check(wga_memset(d.ctx, d_strand, 0, (size_t)n + 16));
  wga_cigar_batch cb;
  cb.d_ops = d_ops;
  cb.d_op_off = d_ooff;
  cb.d_strand_neg = d_strand;
  cb.n_ops = n_ops;
  cb.n = n;
  auto* d_counts = (wga_cigar_counts*)d.alloc((size_t)n * sizeof(wga_cigar_counts));
  auto* d_diag = (wga_rec_diag*)d.alloc((size_t)n * sizeof(wga_rec_diag));
  d.check(wga_cigar_stat(d.ctx, &cb, d_counts, d_diag, nullptr));
  std::vector<wga_rec_diag> diag(n);
  d.download(diag.data(), d_diag, n);
  for (const wga_rec_diag& g : diag)
    if (g.bad_op_idx != WGA_NONE || g.panic_op_idx != WGA_NONE || g.bad_base_pos != WGA_NONE) return leave_to_host();
  g_timer.mark("tokeniser + K1");
  wga_paf_fix_sizes sz;
  d.check(wga_paf_fix(d.ctx, d_text, n_bytes, d_lines, n_lines, d_counts, n_rec, d_work, &sz, nullptr, nullptr, nullptr));
  auto* d_rows = (uint8_t*)d.alloc((size_t)sz.rows_bytes + 16);
  auto* d_ql = (uint8_t*)d.alloc((size_t)sz.qlist_bytes + 16);
  auto* d_tl = (uint8_t*)d.alloc((size_t)sz.tlist_bytes + 16);
  d.check(wga_paf_fix(d.ctx, d_text, n_bytes, d_lines, n_lines, d_counts, n_rec, d_work, &sz, d_rows, d_ql, d_tl));
  download_append(d, acc.q_list, d_ql, (size_t)sz.qlist_bytes);
  download_append(d, acc.t_list, d_tl, (size_t)sz.tlist_bytes);
  download_append(d, acc.rows, d_rows, (size_t)sz.rows_bytes);
  acc.n_total += sz.n_records;
  acc.q_bad += sz.n_q_bad;
  acc.t_bad += sz.n_t_bad;
  d.release_to(owned0);
  g_timer.mark("validate rows (device)");
  return true;
}

int validate_fix_paths(const std::string* input) { /* `__validate_fix_path`: one line per piece */
  Dev d;
  PafChunks chunks(input, true);
  std::string piece;
  uint64_t line0 = 0, byte0 = 0;
  while (chunks.next_text(piece, line0, byte0)) {
    ValidateAcc scratch;
    printf("%s\n", validate_fix_device(d, piece, scratch) ? "device" : "host");
  }
  return 0;
}

/* ---- validate (validate.rs:44-141; SURVEY.md 8f rank 3: free once K1 exists) ------------------------------
 * query_start + M + X + I must be query_end, target_start + M + X + D must be target_end.  Report to the
 * output, optionally all records with corrected ends to --fix.  Lists are in input order (the reference's
 * par_bridge order is not deterministic). */
int cmd_validate(const std::string* input, const std::string* fix, Output& out) {
  Dev d;
  PafChunks chunks(input, fix != nullptr); /* --fix on the host re-serialises every tag: the host reader for those pieces */
  ValidateAcc acc;
  uint64_t &n_total = acc.n_total, &q_bad = acc.q_bad, &t_bad = acc.t_bad;
  std::string &q_list = acc.q_list, &t_list = acc.t_list, &rows = acc.rows;
  WorkerDevices wd(d); /* --gpus N */
  auto host_piece = [&](PafInput& pin) { /* one piece of the file at a time */
    std::vector<PafRecord>& recs = pin.recs;
    const uint32_t n = (uint32_t)recs.size();
    std::vector<wga_cigar_counts> counts(n);
    d.init();
    std::string e;
    if (g_gpus > 1) { /* --gpus N: the records by target hash, as `stat` (the counts meet on the host) */
      try {
        stat_piece_multi(wd.list(), pin, counts);
      } catch (Error& er) {
        e = er.msg;
      }
    } else { /* the tag or tokeniser error speaks before an op K1 rejects */
      std::string op_err;
      e = paf_counts(d, pin, n, counts, op_err);
      if (e.empty()) e = op_err;
    }
    /* rec.get_stat().unwrap() (:79) */
    if (!e.empty()) fail("panic: called `Result::unwrap()` on an `Err` value: " + e);
    n_total += n;
    for (uint32_t k = 0; k < n; k++) {
      PafRecord& r = recs[k];
      const wga_cigar_counts& c = counts[k];
      const uint64_t mx = c.match + c.mismatch;
      const uint64_t eq = r.query_start + mx + c.ins_bp + c.inv_ins_bp, et = r.target_start + mx + c.del_bp + c.inv_del_bp;
      if (eq != r.query_end) {
        q_bad++;
        q_list += r.query_name + ":";
        append_u64(q_list, r.query_start);
        q_list.push_back('-');
        append_u64(q_list, r.query_end);
        q_list.push_back('\n');
        r.query_end = eq;
      }
      if (et != r.target_end) {
        t_bad++;
        t_list += r.target_name + ":";
        append_u64(t_list, r.target_start);
        t_list.push_back('-');
        append_u64(t_list, r.target_end);
        t_list.push_back('\n');
        r.target_end = et;
      }
    }
    if (fix) /* csv writer: tab, flexible, no header; PafRecord field order (paf.rs:50-65) */
      for (const PafRecord& r : recs) {
        append_paf_columns(rows, r.query_name, r.query_length, r.query_start, r.query_end, r.neg, r.target_name, r.target_length,
                           r.target_start, r.target_end, r.matches, r.block_length, r.mapq);
        for (const std::string& tg : r.tags) {
          rows.push_back('\t');
          append_csv_field(rows, tg, '\t');
        }
        rows.push_back('\n');
      }
    d.release_all();
    if (fix) g_timer.mark("validate rows (host)");
  };
  if (fix && g_gpus == 1 && !validate_fix_host_forced()) { /* K29: every piece the plan takes stays on the device */
    std::string piece;
    uint64_t recs_before = 0, line0 = 0, byte0 = 0;
    while (chunks.next_text(piece, line0, byte0)) {
      const uint64_t n_before = acc.n_total;
      if (validate_fix_device(d, piece, acc)) {
        recs_before += acc.n_total - n_before;
        continue;
      }
      PafInput pin;
      pin.recs = parse_paf(piece, recs_before, line0, byte0);
      recs_before += pin.recs.size();
      if (!pin.recs.empty()) host_piece(pin);
    }
  } else {
    PafInput pin;
    while (chunks.next(d, pin)) host_piece(pin);
  }
  std::string text = "Total records: ";
  append_u64(text, n_total);
  text += "\nQuery invalid records: ";
  append_u64(text, q_bad);
  text += "\nTarget invalid records: ";
  append_u64(text, t_bad);
  text += "\nQuery invalid list:\n" + q_list + "Target invalid list:\n" + t_list + "\n"; /* writeln!("{}", ..) */
  out.write(text);
  if (fix) {
    if (*fix == "-") {
      out.write(rows);
    } else {
      Output fo;
      fo.open(*fix, true);
      fo.write(rows);
      fo.close();
    }
  }
  out.close();
  return leave(0);
}
