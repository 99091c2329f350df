/* cmd_pafpseudo.inc — part of wgatools_main.cpp (included there, inside its namespace: the commands share the device helpers, readers and
 * writers defined in front of the include). */
/* ---- pafpseudo (pseudomaf.rs:18-237) ----------------------------------------------------------------
 * Host: grouping by target / query, insertion sort by target_start, gap / overlap / contained
 * logic (:86-95,:147-175,:198-202), and every check that needs no row byte, before anything is written.  GPU: the files' text,
 * built in windows of whole lines of at most WGA_PSEUDO_OUT_BYTES bytes (256 MiB; a longer line is a window of its own): every
 * kept record's segment in target coordinates (gen_pesudo_maf_by_cigar + the head trim, wga_pafpseudo_fill, K6) at its place in
 * the window, and everything around the segments — line heads, the target row, the `-` runs, line ends — by the row frame writer
 * (wga_pafpseudo_frame, K31); the window is streamed into the file and the next one takes its buffer.  An error a window's fill
 * finds (an invalid base, a drain beyond the query) ends the run: the files written so far are complete, the one in progress ends
 * at the last window written.
 * WGA_PSEUDO_WRITER=host: all segments of all targets in one batch, downloaded, and every row put together as a string by one
 * host thread, as before K31 (measurements, and the cross-check of the device writer: same bytes). */
static bool pseudo_host_writer() { return env_is("WGA_PSEUDO_WRITER", "host"); }
static uint64_t pseudo_window_bytes() {
  uint64_t b = (uint64_t)256 << 20;
  if (const char* e = getenv("WGA_PSEUDO_OUT_BYTES")) b = strtoull(e, nullptr, 10);
  return b ? b : 1;
}
struct PseudoSeg {
  size_t rec;        /* index into recs */
  uint64_t gap;      /* '-' columns written before the segment */
  uint64_t overlap;  /* leading columns dropped */
};
struct PseudoQuery {
  std::string name;
  uint64_t size = 0;
  std::vector<size_t> recs; /* sorted by target_start */
  std::vector<PseudoSeg> segs;
  uint64_t tail = 0;
};
struct PseudoTarget {
  std::string name;
  std::vector<size_t> recs;
  std::vector<PseudoQuery> queries;
  uint64_t target_size_first = 0;
};

/* slice::binary_search_by of the Rust std the reference was built with: probe the middle, return
 * at the first equal element [toolchain-dependent for ties: unpinned] */
size_t rust_binary_search_pos(const std::vector<size_t>& v, const std::vector<PafRecord>& recs, uint64_t key) {
  size_t size = v.size(), left = 0, right = size;
  while (left < right) {
    size_t mid = left + size / 2;
    uint64_t probe = recs[v[mid]].target_start;
    if (probe == key) return mid;
    if (probe < key)
      left = mid + 1;
    else
      right = mid;
    size = right - left;
  }
  return left;
}

int cmd_pafpseudo(const std::string* input, const std::string& outdir, bool rewrite, const std::string* fasta,
                  const std::string* only_target) {
  if (outdir == "-") fail("Stdout not allowed here"); /* errors.rs:37 */
  struct stat st;
  if (stat(outdir.c_str(), &st) != 0) {
    /* create_dir_all: every missing component, no shell involved */
    for (size_t k = 1; k <= outdir.size(); k++)
      if (k == outdir.size() || outdir[k] == '/') {
        const std::string part = outdir.substr(0, k);
        if (mkdir(part.c_str(), 0777) != 0 && errno != EEXIST)
          fail("IO error:cannot create directory `" + outdir + "`: " + strerror(errno));
      }
  } else {
    if (!S_ISDIR(st.st_mode)) fail("Path `" + outdir + "` is not a dir");
    if (!rewrite) fail("File `" + outdir + "` already exists, please add `-r` to rewrite it.");
  }
  /* --gpus N: a target's records live on device fnv1a64(target_name) % N (the reference already works target by target,
   * pseudomaf.rs:62-72); every device tokenises, sums and fills its records, the walk and every check run on the host in the
   * reference's processing order, so the first error is the same whatever N is */
  const int ngpu = g_gpus > 1 ? g_gpus : 1;
  std::vector<std::unique_ptr<Dev>> devs;
  for (int g = 0; g < ngpu; g++) devs.emplace_back(new Dev(g));
  Dev& d = *devs[0];
  PafInput pin = load_paf(d, input, false);
  const std::vector<PafRecord>& recs = pin.recs;
  const bool base = fasta != nullptr;
  std::vector<DevFasta> fas(ngpu);
  DevFasta& fa = fas[0]; /* the index (names -> pool offsets) is the same on every device */
  const uint32_t n_all = (uint32_t)recs.size();
  std::vector<uint8_t> has_tag(n_all, 1);
  /* records without a tag are given an empty span so that a device's batch keeps file order */
  if (pin.on_device) {
    for (uint32_t i = 0; i < n_all; i++)
      if (pin.cg_beg[i] == WGA_NONE) {
        has_tag[i] = 0;
        pin.cg_beg[i] = pin.cg_end[i] = 0;
      }
  } else {
    for (uint32_t i = 0; i < n_all; i++) {
      int err = 0;
      (void)paf_cigar_string(recs[i], &err);
      if (err) {
        has_tag[i] = 0;
        pin.recs[i].tags.push_back("cg:Z:"); /* placeholder: tokenises to the empty-CIGAR error, never used */
      }
    }
  }
  std::vector<std::vector<size_t>> mine(ngpu);
  std::vector<uint32_t> owner(n_all, 0), at(n_all, 0); /* record i = record at[i] of device owner[i] */
  for (uint32_t i = 0; i < n_all; i++) {
    const int g = ngpu > 1 ? (int)(fnv1a64(recs[i].target_name) % (uint64_t)ngpu) : 0;
    owner[i] = (uint32_t)g;
    at[i] = (uint32_t)mine[g].size();
    mine[g].push_back(i);
  }
  /* every device: pools, its records' CIGARs tokenised in file order; a record's tag / tokeniser error only counts when
   * the walk below reaches that record (the reference parses a CIGAR when it processes the record) */
  std::vector<CigarTexts> cigars(ngpu);
  std::vector<wga_cigar_batch> cbs(ngpu);
  std::vector<std::vector<wga_tok_err>> terrs(ngpu);
  std::string text16;
  if (pin.on_device && ngpu > 1) text16 = pin.text + std::string(16, '\0');
  std::vector<const uint8_t*> d_texts(ngpu, nullptr); /* the PAF text on device g (a file the device splitter took) */
  std::vector<size_t> keep_front(ngpu, 0);            /* device g's allocations in front of the up-front tokeniser's */
  on_devices(ngpu, [&](int g) {
    Dev& dg = *devs[g];
    cbs[g].n = 0;
    if (base) {
      dg.init();
      fas[g].load(dg, *fasta);
    }
    if (mine[g].empty()) return;
    dg.init();
    const uint8_t* d_text = nullptr;
    if (pin.on_device) d_text = g == 0 ? pin.d_text : dg.upload((const uint8_t*)text16.data(), text16.size());
    d_texts[g] = d_text;
    keep_front[g] = dg.owned.size();
    (void)device_tokenise(dg, pin, 0, (uint32_t)mine[g].size(), cigars[g], &cbs[g], &terrs[g], ngpu > 1 ? mine[g].data() : nullptr,
                          d_text);
  });
  /* 1. group by target (:25-42), then by query with sorted insertion (:86-95) */
  std::vector<PseudoTarget> targets;
  std::unordered_map<std::string, size_t> tindex;
  for (size_t i = 0; i < recs.size(); i++) {
    const PafRecord& r = recs[i];
    if (only_target && r.target_name != *only_target) continue;
    auto it = tindex.find(r.target_name);
    if (it == tindex.end()) {
      it = tindex.emplace(r.target_name, targets.size()).first;
      targets.emplace_back();
      targets.back().name = r.target_name;
    }
    targets[it->second].recs.push_back(i);
  }
  std::vector<uint64_t> q_off(n_all, 0), q_len(n_all, 0), skip(n_all, UINT64_MAX); /* skip = all: a record the walk drops */
  std::vector<uint64_t> walk_pos(n_all, 0); /* a kept record's place in the order the reference processes the records in */
  uint64_t n_kept = 0;
  for (auto& t : targets) {
    std::unordered_map<std::string, size_t> qindex;
    for (size_t i : t.recs) {
      const PafRecord& r = recs[i];
      auto it = qindex.find(r.query_name);
      if (it == qindex.end()) {
        it = qindex.emplace(r.query_name, t.queries.size()).first;
        t.queries.emplace_back();
        t.queries.back().name = r.query_name;
      }
      PseudoQuery& q = t.queries[it->second];
      size_t pos = rust_binary_search_pos(q.recs, recs, r.target_start);
      q.recs.insert(q.recs.begin() + (long)pos, i);
    }
    /* 2. walk (:108-205) */
    uint64_t target_size = 0;
    bool first = true;
    for (auto& q : t.queries) {
      uint64_t last_target_end = 0;
      bool first_query = true;
      for (size_t i : q.recs) {
        const PafRecord& r = recs[i];
        target_size = r.target_length;
        if (first) {
          t.target_size_first = target_size;
          first = false;
        }
        if (first_query) q.size = r.query_length;
        uint64_t overlap = 0, gap = 0;
        if (r.target_start > last_target_end) {
          gap = r.target_start - last_target_end;
        } else {
          if (last_target_end > r.target_end) continue; /* contained: dropped */
          overlap = last_target_end - r.target_start;
        }
        last_target_end = r.target_end;
        uint64_t qo = 0, ql = 0;
        if (base) fa.fetch(q.name, r.query_start, r.query_end - 1, &qo, &ql); /* :222-225 */
        if (!has_tag[i]) fail("CIGAR start tag not found"); /* errors.rs:57 */
        const wga_tok_err& te = terrs[owner[i]][at[i]];
        if (te.err) fail(cigar_error_message(te.err, cigars[owner[i]][at[i]], (size_t)te.tok_off, te.tok_len));
        q_off[i] = qo;
        q_len[i] = ql;
        skip[i] = overlap;
        walk_pos[i] = n_kept++;
        q.segs.push_back(PseudoSeg{i, gap, overlap});
        first_query = false;
      }
      if (last_target_end > target_size)
        fail("panic: attempt to fill a negative tail (pseudomaf.rs:198 underflows)");
      q.tail = target_size - last_target_end;
    }
  }
  /* 3. GPU: class sums -> segment lengths -> fill; a device's batch is its records in file order, dropped records write nothing */
  std::vector<uint64_t> seg_len(n_all, 0), dst_off(n_all, 0); /* dst_off: inside the owner's segment text */
  std::vector<std::string> segs(ngpu);
  if (n_all) {
    std::vector<wga_class_sums> sums(n_all);
    std::vector<wga_class_sums*> d_sums(ngpu, nullptr);
    on_devices(ngpu, [&](int g) {
      const uint32_t n = cbs[g].n;
      if (!n) return;
      Dev& dg = *devs[g];
      d_sums[g] = (wga_class_sums*)dg.alloc((size_t)n * sizeof(wga_class_sums));
      dg.check(wga_cigar_class_sums(dg.ctx, &cbs[g], d_sums[g]));
      std::vector<wga_class_sums> part(n);
      dg.download(part.data(), d_sums[g], n);
      for (uint32_t k = 0; k < n; k++) sums[mine[g][k]] = part[k];
    });
    /* in the order the reference processes the records (an error of an earlier one wins) */
    for (const auto& t : targets)
      for (const auto& q : t.queries)
        for (const auto& sg : q.segs) {
          const size_t k = sg.rec;
          uint64_t len = base ? q_len[k] - (sums[k].i + sums[k].s) + sums[k].d : sums[k].mx + sums[k].d;
          if (base && q_len[k] < sums[k].i + sums[k].s) len = 0; /* reported as a panic below */
          if (skip[k] > len) fail("panic: String::drain range out of bounds (pseudomaf.rs:191)");
          seg_len[k] = len - skip[k];
        }
  }
  if (!pseudo_host_writer()) {
    /* the target rows' slices (base mode), the last of the checks that need no row byte */
    std::vector<uint64_t> t_off(targets.size(), 0), t_len(targets.size(), 0);
    if (base)
      for (size_t ti = 0; ti < targets.size(); ti++)
        if (!targets[ti].queries.empty()) fa.fetch(targets[ti].name, 0, targets[ti].target_size_first - 1, &t_off[ti], &t_len[ti]);
    /* the ops of the whole input have served (tokeniser errors, class sums): a window tokenises its own records again, in the
     * order of its rows, into a batch of its own (DESIGN.md, K31) */
    for (int g = 0; g < ngpu; g++)
      if (devs[g]->ctx && !mine[g].empty()) devs[g]->release_to(keep_front[g]);
    const uint64_t bound = pseudo_window_bytes();
    struct RowsError {
      uint64_t at = UINT64_MAX; /* walk_pos of the record */
      std::string msg;
    };
    std::vector<RowsError> rows_err(ngpu);
    on_devices(ngpu, [&](int g) {
      Dev& dg = *devs[g];
      for (size_t ti = 0; ti < targets.size(); ti++) {
        const PseudoTarget& t = targets[ti];
        if ((ngpu > 1 ? (int)(fnv1a64(t.name) % (uint64_t)ngpu) : 0) != g) continue;
        dg.init();
        /* the file's lines: "a score=0\n", the target row, the query rows, "\n"; a line = its head, its row, '\n' */
        struct Line {
          int kind; /* 0 score, 1 target row, 2 query row, 3 the closing newline */
          size_t q;
          std::string head;
          uint64_t bytes;
        };
        std::vector<Line> lines;
        lines.push_back(Line{0, 0, std::string(), 10});
        auto s_head = [](const std::string& name, uint64_t size) {
          std::string h = "s\t" + name + "\t0\t";
          append_u64(h, size);
          h += "\t+\t";
          append_u64(h, size);
          h.push_back('\t');
          return h;
        };
        if (!t.queries.empty()) {
          Line l{1, 0, s_head(t.name, t.target_size_first), 0};
          l.bytes = l.head.size() + (base ? t_len[ti] : t.target_size_first) + 1;
          lines.push_back(std::move(l));
        }
        for (size_t qi = 0; qi < t.queries.size(); qi++) {
          const PseudoQuery& q = t.queries[qi];
          Line l{2, qi, s_head(q.name, q.size), 0};
          l.bytes = l.head.size() + q.tail + 1;
          for (const auto& sg : q.segs) l.bytes += sg.gap + seg_len[sg.rec];
          lines.push_back(std::move(l));
        }
        lines.push_back(Line{3, 0, std::string(), 1});
        Output out;
        out.open(outdir + "/" + t.name + ".maf", true);
        for (size_t l0 = 0; l0 < lines.size();) {
          size_t l1 = l0 + 1; /* lines [l0, l1): as many whole lines as the bound takes, one at least */
          uint64_t out_bytes = lines[l0].bytes;
          while (l1 < lines.size() && out_bytes + lines[l1].bytes <= bound) out_bytes += lines[l1++].bytes;
          /* the window's items: everything but the segments, which are holes K6 fills */
          std::string blob = "a score=0\n";
          std::vector<wga_span_item> items;
          std::vector<size_t> wrecs; /* the window's kept records, in the order of its rows */
          std::vector<uint64_t> wdst;
          uint64_t at = 0;
          auto put = [&](uint64_t len, uint64_t src, uint32_t kind) {
            if (len) items.push_back(wga_span_item{at, len, src, kind, 0});
            at += len;
          };
          auto put_text = [&](const std::string& text) {
            put(text.size(), blob.size(), WGA_SPAN_COPY_TEXT);
            blob += text;
          };
          for (size_t l = l0; l < l1; l++) {
            const Line& ln = lines[l];
            if (ln.kind == 0) {
              put(10, 0, WGA_SPAN_COPY_TEXT);
              continue;
            }
            if (ln.kind == 1) {
              put_text(ln.head);
              if (base)
                put(t_len[ti], t_off[ti], WGA_SPAN_COPY_POOL);
              else
                put(t.target_size_first, (uint64_t)'N', WGA_SPAN_FILL);
            } else if (ln.kind == 2) {
              const PseudoQuery& q = t.queries[ln.q];
              put_text(ln.head);
              for (const auto& sg : q.segs) {
                put(sg.gap, (uint64_t)'-', WGA_SPAN_FILL);
                wrecs.push_back(sg.rec);
                wdst.push_back(at);
                put(seg_len[sg.rec], 0, WGA_SPAN_HOLE);
              }
              put(q.tail, (uint64_t)'-', WGA_SPAN_FILL);
            }
            put(1, 9, WGA_SPAN_COPY_TEXT); /* the '\n' of "a score=0\n" */
          }
          if (at != out_bytes) fail("internal error: pafpseudo window layout");
          const size_t keep = dg.owned.size();
          dg.out_arena_for((size_t)out_bytes + 64);
          auto* d_win = (uint8_t*)dg.out_arena;
          const uint32_t n = (uint32_t)wrecs.size();
          wga_rec_diag* d_diag = nullptr;
          if (n) {
            CigarTexts wcig;
            wga_cigar_batch wb;
            std::vector<wga_tok_err> werrs;
            (void)device_tokenise(dg, pin, 0, n, wcig, &wb, &werrs, wrecs.data(), d_texts[g]);
            std::vector<uint64_t> qo(n), ql(n), sk(n);
            for (uint32_t k = 0; k < n; k++) qo[k] = q_off[wrecs[k]], ql[k] = q_len[wrecs[k]], sk[k] = skip[wrecs[k]];
            d_diag = (wga_rec_diag*)dg.alloc((size_t)n * sizeof(wga_rec_diag));
            dg.check(wga_pafpseudo_fill(dg.ctx, &wb, base ? 1 : 0, base ? fas[g].d_pool : nullptr, fas[g].bytes,
                                        base ? dg.upload(qo) : nullptr, base ? dg.upload(ql) : nullptr, dg.upload(sk), d_win,
                                        dg.upload(wdst), d_diag));
          }
          auto* d_bad = (uint64_t*)dg.alloc(8);
          blob.append(16, '\0');
          dg.check(wga_pafpseudo_frame(dg.ctx, items.size(), dg.upload(items), base ? fas[g].d_pool : nullptr, base ? fas[g].bytes : 0,
                                       dg.upload((const uint8_t*)blob.data(), blob.size()), blob.size() - 16, d_win, out_bytes, d_bad));
          uint64_t bad = 0;
          dg.download(&bad, d_bad, 1);
          if (bad != WGA_NONE) fail("internal error: pafpseudo window item " + std::to_string(bad));
          if (n) { /* in the order the reference processes the records: the window's own */
            std::vector<wga_rec_diag> diag(n);
            dg.download(diag.data(), d_diag, n);
            for (uint32_t k = 0; k < n && rows_err[g].msg.empty(); k++) {
              const size_t i = wrecs[k];
              if (diag[k].bad_base_pos != WGA_NONE)
                rows_err[g].msg = std::string("Invalid Base: `") + fas[g].at(dg, q_off[i] + q_len[i] - 1 - diag[k].bad_base_pos) + "`";
              else if (diag[k].panic_op_idx != WGA_NONE)
                rows_err[g].msg = "panic: String::drain / insert_str beyond the end of the query sequence (cigar.rs:772,779)";
              if (!rows_err[g].msg.empty()) rows_err[g].at = walk_pos[i];
            }
          }
          if (!rows_err[g].msg.empty()) break; /* the file ends at the last window written */
          stream_out(dg, out, d_win, (size_t)out_bytes, false);
          dg.release_to(keep);
          l0 = l1;
        }
        out.close();
        if (!rows_err[g].msg.empty()) return;
      }
    });
    g_timer.mark("pafpseudo rows (device)");
    int first = -1; /* the device whose error the reference would have met first */
    for (int g = 0; g < ngpu; g++)
      if (!rows_err[g].msg.empty() && (first < 0 || rows_err[g].at < rows_err[first].at)) first = g;
    if (first >= 0) fail(rows_err[first].msg);
    return leave(0);
  }
  /* WGA_PSEUDO_WRITER=host: one fill of every kept segment of every target, the rows put together on the host */
  if (n_all) {
    std::vector<std::vector<wga_rec_diag>> diag(ngpu);
    on_devices(ngpu, [&](int g) {
      const uint32_t n = cbs[g].n;
      if (!n) return;
      Dev& dg = *devs[g];
      std::vector<uint64_t> qo(n), ql(n), sk(n), doff(n + 1, 0);
      for (uint32_t k = 0; k < n; k++) {
        const size_t i = mine[g][k];
        qo[k] = q_off[i], ql[k] = q_len[i], sk[k] = skip[i];
        dst_off[i] = doff[k];
        doff[k + 1] = doff[k] + seg_len[i];
      }
      auto* d_out = (uint8_t*)dg.alloc(doff[n] + 64);
      auto* d_diag = (wga_rec_diag*)dg.alloc((size_t)n * sizeof(wga_rec_diag));
      uint8_t* d_pool = base ? fas[g].d_pool : nullptr;
      dg.check(wga_pafpseudo_fill(dg.ctx, &cbs[g], base ? 1 : 0, d_pool, fas[g].bytes, base ? dg.upload(qo) : nullptr,
                                  base ? dg.upload(ql) : nullptr, dg.upload(sk), d_out, dg.upload(doff), d_diag));
      diag[g].resize(n);
      dg.download(diag[g].data(), d_diag, n);
      segs[g].resize(doff[n]);
      if (doff[n]) dg.download((uint8_t*)segs[g].data(), d_out, doff[n]);
    });
    for (const auto& t : targets)
      for (const auto& q : t.queries)
        for (const auto& sg : q.segs) {
          const size_t k = sg.rec;
          const wga_rec_diag& dk = diag[owner[k]][at[k]];
          if (dk.bad_base_pos != WGA_NONE)
            fail(std::string("Invalid Base: `") + fas[owner[k]].at(*devs[owner[k]], q_off[k] + q_len[k] - 1 - dk.bad_base_pos) + "`");
          if (dk.panic_op_idx != WGA_NONE)
            fail("panic: String::drain / insert_str beyond the end of the query sequence (cigar.rs:772,779)");
        }
  }
  /* 4. one file per target (:62-72, :98-209) */
  for (const auto& t : targets) {
    Output out;
    out.open(outdir + "/" + t.name + ".maf", true);
    std::string text = "a score=0\n";
    if (!t.queries.empty()) {
      text += "s\t" + t.name + "\t0\t";
      append_u64(text, t.target_size_first);
      text += "\t+\t";
      append_u64(text, t.target_size_first);
      text.push_back('\t');
      if (base) {
        uint64_t o, l;
        fa.fetch(t.name, 0, t.target_size_first - 1, &o, &l);
        text += fa.slice(d, o, l);
      } else {
        text.append(t.target_size_first, 'N');
      }
      text.push_back('\n');
    }
    for (const auto& q : t.queries) {
      text += "s\t" + q.name + "\t0\t";
      append_u64(text, q.size);
      text += "\t+\t";
      append_u64(text, q.size);
      text.push_back('\t');
      for (const auto& sg : q.segs) {
        text.append(sg.gap, '-');
        text.append(segs[owner[sg.rec]], dst_off[sg.rec], seg_len[sg.rec]);
      }
      text.append(q.tail, '-');
      text.push_back('\n');
      if (text.size() > (1u << 26)) {
        out.write(text);
        text.clear();
      }
    }
    text.push_back('\n');
    out.write(text);
    out.close();
  }
  g_timer.mark("pafpseudo rows (host)");
  return leave(0);
}
