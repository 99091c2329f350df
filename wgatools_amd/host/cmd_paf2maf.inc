/* cmd_paf2maf.inc — part of wgatools_main.cpp (included there, inside its namespace: the commands share the device helpers, readers and
 * writers defined in front of the include). */
/* ---- paf2maf (converter.rs:176-265) ------------------------------------------------------------- */
/* fnv1a64(name): the sharding rule of the multi-device paths (the same hash as wgatools_amd/shard.py) */
static uint64_t fnv1a64(const std::string& s) {
  uint64_t h = 0xCBF29CE484222325ull;
  for (unsigned char c : s) h = (h ^ c) * 0x100000001B3ull;
  return h;
}

/* The body of the converter's record loop over records which[0 .. n_which) of a piece (which == nullptr: all of them), in
 * resident batches: slices fetched (target first, then query: converter.rs:219-225), CIGARs tokenised on the device, rows
 * expanded, text handed to the sink.  Returns the position (in `which` order) of the first failing record, or n_which;
 * `err` = the reference's message for it. */
size_t p2m_run(Dev& d, DevFasta& tf, DevFasta& qf, const PafInput& in, const size_t* which, size_t n_which,
               const uint8_t* d_text_here, BatchSink sink, std::string& err) {
  const std::vector<PafRecord>& recs = in.recs;
  auto rec_of = [&](size_t k) -> const PafRecord& { return recs[which ? which[k] : k]; };
  const uint64_t kMaxBytes = 6ull << 30;
  const uint64_t kMaxText = 160ull << 20; /* ~64 M ops */
  const size_t keep = d.owned.size();
  size_t i0 = 0;
  while (i0 < n_which && err.empty()) {
    ExpandJob job;
    uint64_t est = 0, est_text = 0;
    size_t i = i0;
    for (; i < n_which; i++) {
      const PafRecord& r = rec_of(i);
      if (i > i0 && (est_text > kMaxText || est > kMaxBytes)) break;
      uint64_t to, tl, qo, ql;
      try { /* fetch order of converter.rs:219-225: target first, then query */
        tf.fetch(r.target_name, r.target_start, r.target_end - 1, &to, &tl);
        qf.fetch(r.query_name, r.query_start, r.query_end - 1, &qo, &ql);
      } catch (Error& e) {
        err = e.msg;
        break;
      }
      est_text += in.cigar_bytes(which ? which[i] : i);
      job.add(to, tl, qo, ql, r.mapq, r.target_name, r.target_start, r.target_end - r.target_start, false,
              r.target_length, r.query_name, r.neg ? r.query_length - r.query_end : r.query_start, /* converter.rs:213-216 */
              r.query_end - r.query_start, r.neg, r.query_length);
      est += tl + ql + (tl + ql) / 4;
    }
    size_t bad_at = err.empty() ? n_which : i; /* a fetch error belongs to record i */
    /* the CIGARs of records [i0, i) are tokenised on the device; a tag / tokeniser error cuts the
     * batch before the failing record (reverse_complement runs before the CIGAR is looked at, so
     * an invalid base in that record's query slice still wins: checked on the host, rare path) */
    CigarTexts cigars;
    wga_cigar_batch cb;
    cb.n = 0;
    if (i > i0) {
      const std::string terr = device_tokenise(d, in, i0, (uint32_t)(i - i0), cigars, &cb, nullptr, which, d_text_here);
      if (!terr.empty()) {
        const size_t k = cb.n;
        std::string perr = terr;
        const PafRecord& r = rec_of(i0 + k);
        if (r.neg) {
          const std::string qs = qf.slice(d, job.q_off[k], job.q_len[k]);
          for (uint64_t x = job.q_len[k]; x-- > 0;) {
            char c = qs[x];
            if (!strchr("ACGTNacgtn", c) || c == 0) {
              perr = std::string("Invalid Base: `") + c + "`";
              break;
            }
          }
        }
        err = perr;
        i = i0 + k;
        bad_at = i;
      }
    }
    const uint32_t n = cb.n;
    if (n) {
      job.resize(n);
      wga_rec_diag g;
      sink.which = which;
      sink.first = i0;
      sink.records_phase = kPaf2mafRecords;
      const uint32_t good = expand_batch(d, cb, job, tf.d_pool, tf.bytes, qf.d_pool, qf.bytes, sink, &g);
      if (good < n) {
        const uint32_t k = good;
        if (g.bad_base_pos != WGA_NONE) { /* utils.rs:97 */
          char c = qf.at(d, job.q_off[k] + job.q_len[k] - 1 - g.bad_base_pos);
          err = std::string("Invalid Base: `") + c + "`";
        } else if (g.bad_op_idx < g.panic_op_idx) { /* errors.rs:59 */
          err = "CIGAR OP `" + cigar_op_token_at(cigars[k], g.bad_op_idx) + "` invalid";
        } else {
          err = "panic: String::insert_str beyond the end of the fetched sequence (cigar.rs:507,513)";
        }
        bad_at = i0 + k;
      }
    }
    d.release_to(keep); /* this batch's buffers */
    if (!err.empty()) return bad_at;
    i0 = i;
  }
  return n_which;
}

/* `wgatools --gpus N paf2maf`: a piece of the PAF is framed once (device 0 splits it), every record belongs to device
 * fnv1a64(target_name) % N, and N worker threads — one context, one pair of sequence pools each — run the same record loop
 * over their share: a first pass for the byte count of every record (K1 + the layout scan; no row byte yet), then, with the
 * file offsets those sizes give in INPUT order, a second pass that expands the rows and pwrite()s every record where it
 * belongs.  No row byte crosses devices; the first failing record in input order ends the run and the file ends in front
 * of it, as the reference's serial loop leaves it (converter.rs:196-263). */
int cmd_paf2maf_multi(const std::string* input, const std::string& t_fa, const std::string& q_fa, Output& out, int ngpu) {
  std::vector<std::unique_ptr<Dev>> devs;
  for (int g = 0; g < ngpu; g++) devs.emplace_back(new Dev(g));
  PafChunks chunks(input, false);
  std::vector<DevFasta> tf(ngpu), qf(ngpu);
  auto on_all = [&](const std::function<void(int)>& fn) { on_devices(ngpu, fn); };
  on_all([&](int g) {
    devs[g]->init();
    tf[g].load(*devs[g], t_fa);
    qf[g].load(*devs[g], q_fa);
  });
  g_timer.mark("fasta read + device pools");
  std::vector<size_t> keep_pools(ngpu);
  for (int g = 0; g < ngpu; g++) keep_pools[g] = devs[g]->owned.size(); /* the pools stay for the whole run */
  out.write("#maf version=1.6 convert_from=paf t_seq_path=" + t_fa + " q_seq_path=" + q_fa + "\n");
  uint64_t pos0 = 0;
  const int fd = out.plain_fd(&pos0);
  if (fd < 0) fail("internal error: --gpus needs a plain output file");
  uint64_t file_pos = pos0;
  std::string pending_error;
  PafInput in;
  for (;;) {
    bool more = false;
    try {
      more = chunks.next(*devs[0], in);
    } catch (Error& e) {
      pending_error = e.msg;
    }
    g_timer.mark("paf read + upload + split");
    if (!more) break;
    const size_t n = in.recs.size();
    std::vector<std::vector<size_t>> mine(ngpu);
    for (size_t i = 0; i < n; i++) mine[fnv1a64(in.recs[i].target_name) % (uint64_t)ngpu].push_back(i);
    std::vector<const uint8_t*> d_text(ngpu, nullptr);
    std::vector<uint64_t> sizes(n, 0), offsets(n + 1, 0);
    std::vector<size_t> bad_at(ngpu, n); /* input index of a worker's first failing record */
    std::vector<std::string> bad_msg(ngpu);
    std::string text16;
    if (in.on_device && ngpu > 1) text16 = in.text + std::string(16, '\0');
    auto pass = [&](BatchSink::Mode mode, size_t upto) {
      on_all([&](int g) {
        Dev& d = *devs[g];
        if (in.on_device && !d_text[g])
          d_text[g] = g == 0 ? in.d_text : d.upload((const uint8_t*)text16.data(), text16.size());
        std::vector<size_t>& w = mine[g];
        size_t cnt = std::lower_bound(w.begin(), w.end(), upto) - w.begin(); /* records in front of the first known error */
        BatchSink sink;
        sink.mode = mode;
        sink.sizes = &sizes;
        sink.offsets = &offsets;
        sink.fd = fd;
        std::string err;
        const size_t k = p2m_run(d, tf[g], qf[g], in, w.data(), cnt, d_text[g], sink, err);
        if (k < cnt && w[k] < bad_at[g]) {
          bad_at[g] = w[k];
          bad_msg[g] = err;
        }
      });
    };
    pass(BatchSink::SIZES, n);
    size_t first_bad = n;
    for (int g = 0; g < ngpu; g++) first_bad = std::min(first_bad, bad_at[g]);
    offsets[0] = file_pos;
    for (size_t i = 0; i < n; i++) offsets[i + 1] = offsets[i] + (i < first_bad ? sizes[i] : 0);
    g_timer.mark("sizes (K1 + layout on every device)");
    pass(BatchSink::ROWS, first_bad);
    for (int g = 0; g < ngpu; g++) first_bad = std::min(first_bad, bad_at[g]);
    g_timer.mark("rows + copy out + write");
    g_timer.mark(kPaf2mafRecords[maf_frame_host_writer() ? 1 : 0]); /* the devices' workers do not mark: this names the writer they ran */
    file_pos = offsets[first_bad];
    for (int g = 0; g < ngpu; g++) devs[g]->release_to(keep_pools[g]); /* the piece's text on every device */
    if (first_bad < n) {
      for (int g = 0; g < ngpu; g++)
        if (bad_at[g] == first_bad) pending_error = bad_msg[g];
      break;
    }
  }
  /* the file ends behind the last record in front of the first failing one (later records of other devices may have
   * been written beyond it) */
  if (ftruncate(fd, (off_t)file_pos) != 0) fail("IO error:truncate failed");
  out.advance(file_pos - pos0);
  out.close();
  if (!pending_error.empty()) fail(pending_error);
  return leave(0);
}

int cmd_paf2maf(const std::string* input, const std::string& t_fa, const std::string& q_fa, Output& out) {
  {
    uint64_t pos = 0;
    if (g_gpus > 1 && out.plain_fd(&pos) >= 0) return cmd_paf2maf_multi(input, t_fa, q_fa, out, g_gpus);
  }
  Dev d;
  PafChunks chunks(input, false); /* the input is opened first, then the two indexed FASTA files (utils.rs, converter.rs:183-186) */
  DevFasta tf, qf;
  d.init();
  tf.load(d, t_fa);
  qf.load(d, q_fa);
  g_timer.mark("fasta read + device pools");
  out.write("#maf version=1.6 convert_from=paf t_seq_path=" + t_fa + " q_seq_path=" + q_fa + "\n");
  const size_t keep_pools = d.owned.size(); /* the pools stay for the whole run */
  std::string pending_error;
  PafInput in;
  /* the input streams through in pieces (records before a failing one are written, like the reference's reader loop) */
  for (;;) {
    bool more = false;
    g_timer.mark("host");
    try {
      more = chunks.next(d, in);
    } catch (Error& e) {
      pending_error = e.msg;
    }
    g_timer.mark("paf read + upload + split");
    if (!more) break;
    BatchSink sink;
    sink.out = &out;
    p2m_run(d, tf, qf, in, nullptr, in.recs.size(), nullptr, sink, pending_error);
    g_timer.mark(kPaf2mafRecords[maf_frame_host_writer() ? 1 : 0]); /* a piece without a record to write */
    d.release_to(keep_pools);
    if (!pending_error.empty()) break;
  }
  out.close();
  if (!pending_error.empty()) fail(pending_error);
  return leave(0);
}
