/* cmd_maf2paf.inc — part of wgatools_main.cpp (included there, inside its namespace: the commands share the device helpers, readers and
 * writers defined in front of the include). */
/* ---- maf2paf (converter.rs:29-54, maf.rs:484-520) ------------------------------------------------ */
/* WGA_MAF2PAF_WRITER=host: the records' fields are printed by host threads around the device's cg:Z: text, as before K28
 * (measurements, and the cross-check of the device writer: same bytes) */
static bool maf2paf_host_writer() { return env_is("WGA_MAF2PAF_WRITER", "host"); }

/* the PAF rows of blocks recs[0 .. n), whose rows stand on device d (p).  The records are written on the device (wga_maf2paf,
 * K28): the host fills the numbers of every head and says where the two names stand — in the uploaded file where the device
 * splitter took the piece and d holds it (p.names_in_rows), otherwise in a buffer the range's names are gathered in.  Only the
 * number of runs and the text's length come back before the text. */
static std::string maf2paf_rows(Dev& d, const MafRows& p, const MafRecord* const* recs, uint32_t n, bool host_writer) {
  std::string text;
  const MafRuns R = maf_runs(d, p, n);
  if (!host_writer && (uint64_t)n + R.n_runs <= 0xFFFFFFF0ull) { /* beyond wga_maf2paf's limit: the host's fields */
    RecordHeads hd(n, &p);
    for (uint32_t k = 0; k < n; k++) hd.add(*recs[k]);
    hd.upload(d);
    const DevText t = two_call_text(d, (size_t)wga_maf2paf_work_bytes(n, R.n_runs), [&](void* d_work, uint64_t* total, uint8_t* d_out) {
      return wga_maf2paf(d.ctx, n, hd.d_names, hd.n_name_bytes, hd.d_heads, R.d_counts, R.d_runs, R.d_roff, p.d_c, d_work, total, d_out);
    });
    text.resize(t.bytes);
    if (t.bytes) d.download((uint8_t*)&text[0], t.d_out, t.bytes);
    return text;
  }
  std::vector<uint64_t> roff(n + 1);
  d.download(roff.data(), R.d_roff, n + 1);
  /* the cg:Z: text is formatted on the device (wga_maf_runs_cigar_text) between the host's fields */
  auto* d_tb = (uint64_t*)d.alloc((size_t)n * 8);
  d.check(wga_maf_runs_cigar_text(d.ctx, n, roff[n], R.d_runs, R.d_roff, p.d_c, d_tb, nullptr, nullptr));
  std::vector<uint64_t> tb(n);
  d.download(tb.data(), d_tb, n);
  std::vector<wga_cigar_counts> counts(n);
  d.download(counts.data(), R.d_counts, n);
  /* the fields around the cg:Z: text: a record's "<12 columns>\tNM:i:<n>\tcg:Z:" and its "\n", formatted by host threads over
   * contiguous ranges of blocks (2 000 000 blocks: 0.5 s on one thread), dropped into the output by wga_scatter_bytes */
  unsigned nthr = std::thread::hardware_concurrency();
  nthr = std::max(1u, std::min({nthr, 32u, n / 4096u + 1u}));
  std::vector<std::string> blobs(nthr);
  std::vector<uint32_t> hsize(n);
  auto fmt = [&](unsigned t) {
    const uint32_t lo = (uint32_t)((uint64_t)n * t / nthr), hi = (uint32_t)((uint64_t)n * (t + 1) / nthr);
    std::string& bl = blobs[t];
    bl.reserve((size_t)(hi - lo) * 96);
    for (uint32_t k = lo; k < hi; k++) {
      const MafRecord& r = *recs[k];
      const wga_cigar_counts& c = counts[k];
      const uint64_t block = c.match + c.mismatch + c.ins_bp + c.inv_ins_bp + c.del_bp + c.inv_del_bp;
      const size_t at = bl.size();
      append_paf_columns(bl, r.q().name, r.q().size, r.query_start(), r.query_end(), r.q().neg, r.t().name, r.t().size, r.t().start,
                         r.t().start + r.t().align_size, c.match, block);
      bl += "\tNM:i:";
      append_u64(bl, block - c.match);
      bl += "\tcg:Z:";
      hsize[k] = (uint32_t)(bl.size() - at);
      bl.push_back('\n');
    }
  };
  {
    std::vector<std::thread> th;
    for (unsigned t = 1; t < nthr; t++) th.emplace_back(fmt, t);
    fmt(0);
    for (auto& x : th) x.join();
  }
  HostFraming f; /* the threads' blobs joined are its blob: a head, then the "\n" behind the cg:Z: text, per record */
  {
    size_t total = 0;
    for (const std::string& bl : blobs) total += bl.size();
    f.blob.reserve(total);
    for (const std::string& bl : blobs) f.blob += bl;
  }
  for (uint32_t k = 0; k < n; k++) f.place(hsize[k], tb[k], 1);
  auto* d_out = (uint8_t*)d.alloc(f.pos + 64);
  d.check(wga_maf_runs_cigar_text(d.ctx, n, roff[n], R.d_runs, R.d_roff, p.d_c, nullptr, d_out, d.upload(f.mid_off)));
  f.scatter(d, d_out);
  text.resize((size_t)f.pos);
  if (f.pos) d.download((uint8_t*)&text[0], d_out, f.pos);
  return text;
}

int cmd_maf2paf(const std::string* input, const std::string* query_name, Output& out) {
  Dev d;
  MafDevices md(d); /* --gpus N: a piece's blocks in contiguous ranges over the devices, the rows meet in block order */
  MafChunks chunks(input);
  const bool host_writer = maf2paf_host_writer();
  std::vector<std::string> all_text; /* converter.rs:40-52 collects every record before it writes the first: an error leaves no output
                                        (the pieces' rows are kept as they come — no 0.4 GB concatenation — and written at the end) */
  MafInput min;
  g_timer.mark("host");
  while (chunks.next(d, min)) {
    g_timer.mark("read + upload + split");
    std::vector<MafRecord>& recs = min.recs;
    select_query(recs, query_name);
    if (!recs.empty()) {
      const std::vector<const MafRecord*> all = all_records(recs);
      std::vector<std::string> part(md.count());
      md.run(min, all, false, [&](int g, Dev& dg, const MafRows& p, uint32_t lo, uint32_t cnt) {
        part[g] = maf2paf_rows(dg, p, all.data() + lo, cnt, host_writer);
      });
      g_timer.mark(host_writer ? "maf2paf records (host)" : "maf2paf records (device)");
      for (std::string& t : part) all_text.push_back(std::move(t));
    }
    md.release_all();
  }
  for (const std::string& t : all_text) out.write(t);
  g_timer.mark("write");
  out.close();
  return leave(0);
}
