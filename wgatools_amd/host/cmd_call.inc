/* cmd_call.inc — part of wgatools_main.cpp (included there, inside its namespace: the commands share the device helpers, readers and
 * writers defined in front of the include). */
/* ---- call (MAF) (caller.rs:42-265, 388-608) ------------------------------------------------------------
 * GPU: the column walk — runs of equal caller class with non-gap prefix counts (wga_maf_call_runs) — and, on that run list
 * where it lies, the SV-safe chunk cuts, the chunk coordinates, the after_m event rules, the REF / ALT bases and the VCF
 * text (wga_maf_call_vcf; noodles-vcf 0.43 layout, README.md:323-343).  Host: which blocks are called (:62-108), the
 * header, and the text's way out. */

/* build_header, caller.rs:304-338 as noodles-vcf 0.43 prints it (README.md:323-331) */
std::string vcf_header(const std::string& sample, const std::vector<std::pair<std::string, uint64_t>>& contigs) {
  std::string h =
      "##fileformat=VCFv4.4\n"
      "##INFO=<ID=SVLEN,Number=A,Type=Integer,Description=\"Length of structural variant\">\n"
      "##INFO=<ID=SVTYPE,Number=1,Type=String,Description=\"Type of structural variant\">\n"
      "##INFO=<ID=END,Number=1,Type=Integer,Description=\"End position of the longest variant described in this record\">\n"
      "##INFO=<ID=INV_NEST,Number=1,Type=String,Description=\"Varations nested within inversion\">\n"
      "##FORMAT=<ID=QI,Number=1,Type=String,Description=\"Query informations\">\n"
      "##FORMAT=<ID=GT,Number=1,Type=String,Description=\"Genotype\">\n";
  for (auto& c : contigs) { /* add_header_contig :340-357; placement after FORMAT is unpinned */
    h += "##contig=<ID=" + c.first + ",length=";
    append_u64(h, c.second);
    h += ">\n";
  }
  h += "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\t" + sample + "\n";
  return h;
}

/* ---- call (PAF) (caller.rs:268-302, 610-822) -----------------------------------------------------------
 * GPU: the op walk (wga_paf_call_events) and the event -> VCF row text (wga_paf_call_vcf).  Host: fetch coordinates. */
/* the records which[0 .. n_which) of a piece (which == nullptr: all of them) in resident batches; their VCF rows are
 * appended to `body` in that order (`sizes`, when given, gets every record's byte count).  Errors are thrown; *bad_at is then
 * the position (in `which` order) of the record they belong to. */
void call_paf_run(Dev& d, DevFasta& tf, DevFasta& qf, const PafInput& pin, const size_t* which, size_t n_which,
                  const uint8_t* d_text_here, bool snp, uint64_t svlen, std::string& body, std::vector<uint64_t>* sizes,
                  size_t* bad_at) {
  const std::vector<PafRecord>& recs = pin.recs;
  const size_t keep = d.owned.size(); /* the input text, the pools */
  const uint64_t kMaxText = 160ull << 20; /* ~64 M ops per batch */
  size_t i0 = 0;
  while (i0 < n_which) {
    std::vector<uint64_t> t_off, t_len, q_off, q_len;
    size_t i = i0;
    uint64_t est_text = 0;
    for (; i < n_which; i++) {
      const size_t ri = which ? which[i] : i;
      const PafRecord& r = recs[ri];
      *bad_at = i; /* an error raised from here on belongs to this record */
      if (i > i0 && est_text > kMaxText) break;
      uint64_t to, tl, qo, ql;
      tf.fetch(r.target_name, r.target_start, r.target_end, &to, &tl); /* paf.rs:221-237: end inclusive */
      qf.fetch(r.query_name, r.query_start, r.query_end, &qo, &ql);
      if (r.neg && tl == 0) fail("panic: byte index 1 is out of bounds of the fetched target (caller.rs:642)");
      { /* a missing tag or an empty CIGAR ends the run at this record (checked here to keep the order of the errors) */
        bool has_tag, empty;
        if (pin.on_device) {
          has_tag = pin.cg_beg[ri] != WGA_NONE;
          empty = has_tag && pin.cg_end[ri] == pin.cg_beg[ri];
        } else {
          int err = 0;
          const std::string cg = paf_cigar_string(r, &err);
          has_tag = !err;
          empty = has_tag && cg.size() == 5;
        }
        if (!has_tag) fail("CIGAR start tag not found");
        if (empty) fail(cigar_error_message(WGA_REC_PANIC, std::string(), 0, 0));
      }
      est_text += pin.cigar_bytes(ri);
      t_off.push_back(to);
      t_len.push_back(tl);
      q_off.push_back(qo);
      q_len.push_back(ql);
    }
    /* the CIGARs are tokenised on the device; tokeniser errors end a record's walk but are discarded
     * (:673,815-819): the ops in front of them are kept.  Only a missing tag and an empty CIGAR are fatal. */
    CigarTexts cigars;
    wga_cigar_batch cb;
    std::vector<wga_tok_err> terrs;
    const uint32_t n_asked = (uint32_t)(i - i0);
    const std::string tag_err = device_tokenise(d, pin, i0, n_asked, cigars, &cb, &terrs, which, d_text_here);
    for (uint32_t k = 0; k < cb.n; k++)
      if (terrs[k].err == WGA_REC_PANIC) {
        *bad_at = i0 + k;
        fail(cigar_error_message(WGA_REC_PANIC, std::string(), 0, 0));
      }
    *bad_at = i0 + cb.n;
    if (cb.n < n_asked) fail(tag_err); /* records are processed in order: the first failing one ends the run */
    const uint32_t n = cb.n;
    if (n) {
      auto* d_cnt = (uint64_t*)d.alloc((size_t)n * 8);
      d.check(wga_paf_call_events(d.ctx, &cb, svlen, snp, d_cnt, nullptr, nullptr));
      uint64_t n_ev = 0;
      uint64_t* d_eoff = d.scan(n, d_cnt, &n_ev);
      auto* d_ev = (uint64_t*)d.alloc((3 * n_ev + 3) * 8);
      d.check(wga_paf_call_events(d.ctx, &cb, svlen, snp, d_cnt, d_ev, d_eoff));
      /* the rows are formatted where the events lie (wga_paf_call_vcf): names, coordinates and the places of the fetched
       * sequences go up, the text comes back; the driver is buffered, so an error in any record leaves nothing written
       * (:294-299) */
      std::string names;
      std::unordered_map<std::string, uint64_t> name_at;
      auto name_off = [&](const std::string& nm) {
        auto it = name_at.find(nm);
        if (it != name_at.end()) return it->second;
        const uint64_t at = names.size();
        names += nm;
        name_at.emplace(nm, at);
        return at;
      };
      std::vector<wga_vcf_rec> vr(n);
      for (uint32_t k = 0; k < n; k++) {
        const PafRecord& r = recs[which ? which[i0 + k] : i0 + k];
        wga_vcf_rec& v = vr[k];
        v.t_name_off = name_off(r.target_name), v.t_name_len = (uint32_t)r.target_name.size();
        v.q_name_off = name_off(r.query_name), v.q_name_len = (uint32_t)r.query_name.size();
        v.t_start = r.target_start, v.t_end = r.target_end, v.q_start = r.query_start, v.q_end = r.query_end;
        v.t_off = t_off[k], v.t_len = t_len[k], v.q_off = q_off[k], v.q_len = q_len[k];
      }
      names.push_back('\0'); /* never empty */
      const uint8_t* d_names = d.upload((const uint8_t*)names.data(), names.size());
      const wga_vcf_rec* d_vr = d.upload(vr.data(), vr.size());
      auto* d_nb = (uint64_t*)d.alloc((size_t)n * 8);
      auto* d_err = (wga_vcf_err*)d.alloc((size_t)n * sizeof(wga_vcf_err));
      d.check(wga_paf_call_vcf(d.ctx, &cb, svlen, d_ev, d_eoff, d_vr, d_names, tf.d_pool, qf.d_pool, d_nb, d_err, nullptr,
                               nullptr));
      auto* d_toff = (uint64_t*)d.alloc(((size_t)n + 1) * 8);
      d.check(wga_exclusive_scan_u64(d.ctx, n, d_nb, d_toff));
      std::vector<wga_vcf_err> errs(n);
      d.download(errs.data(), (const wga_vcf_err*)d_err, n);
      for (uint32_t k = 0; k < n; k++) { /* the first failing record in input order */
        if (errs[k].item == WGA_NONE) continue;
        *bad_at = i0 + k;
        if (errs[k].kind == 1)
          fail("panic: VCF REF/ALT slice out of the fetched sequence (caller.rs:695-696,753-754,800-801)");
        fail(std::string("invalid reference/alternate base `") + (char)errs[k].ch +
             "` for a VCF record (noodles-vcf parse error)");
      }
      uint64_t n_text = 0;
      d.download(&n_text, (const uint64_t*)d_toff + n, 1);
      if (sizes) {
        std::vector<uint64_t> nb(n);
        d.download(nb.data(), (const uint64_t*)d_nb, n);
        sizes->insert(sizes->end(), nb.begin(), nb.end());
      }
      if (n_text) {
        auto* d_text = (uint8_t*)d.alloc(n_text + 64);
        d.check(wga_paf_call_vcf(d.ctx, &cb, svlen, d_ev, d_eoff, d_vr, d_names, tf.d_pool, qf.d_pool, nullptr, nullptr,
                                 d_text, d_toff));
        const size_t at = body.size();
        body.resize(at + n_text);
        d.download((uint8_t*)&body[at], (const uint8_t*)d_text, n_text);
      }
    }
    d.release_to(keep);
    i0 = i;
  }
  *bad_at = n_which;
}

int cmd_call_paf_multi(const std::string* input, const std::string& t_fa, const std::string& q_fa, bool snp, uint64_t svlen,
                       const std::string& sample, Output& out, int ngpu) {
  /* --gpus N: the records go to the devices by fnv1a64(target_name) % N; every device walks and formats its share, the rows
   * meet on the host in input order (the driver is buffered: caller.rs:294-299); the first failing record in input order
   * decides the message */
  std::vector<std::unique_ptr<Dev>> devs;
  for (int g = 0; g < ngpu; g++) devs.emplace_back(new Dev(g));
  PafInput pin = load_paf(*devs[0], input, false);
  const size_t n = pin.recs.size();
  std::vector<DevFasta> tf(ngpu), qf(ngpu);
  std::vector<std::vector<size_t>> mine(ngpu);
  for (size_t i = 0; i < n; i++) mine[fnv1a64(pin.recs[i].target_name) % (uint64_t)ngpu].push_back(i);
  std::string text16;
  if (pin.on_device && ngpu > 1) text16 = pin.text + std::string(16, '\0');
  std::vector<std::string> bodies(ngpu), msgs(ngpu);
  std::vector<std::vector<uint64_t>> sizes(ngpu);
  std::vector<size_t> bad(ngpu, n); /* input index of a worker's failing record */
  on_devices(ngpu, [&](int g) {
    Dev& d = *devs[g];
    size_t at = 0;
    try {
      d.init();
      tf[g].load(d, t_fa);
      qf[g].load(d, q_fa);
      const uint8_t* d_text = nullptr;
      if (pin.on_device) d_text = g == 0 ? pin.d_text : d.upload((const uint8_t*)text16.data(), text16.size());
      call_paf_run(d, tf[g], qf[g], pin, mine[g].data(), mine[g].size(), d_text, snp, svlen, bodies[g], &sizes[g], &at);
    } catch (Error& e) {
      bad[g] = at < mine[g].size() ? mine[g][at] : (mine[g].empty() ? 0 : mine[g].back());
      msgs[g] = e.msg.empty() ? std::string("error") : e.msg;
    } catch (std::exception& e) { /* bad_alloc and friends: an exception leaving a thread is std::terminate */
      bad[g] = at < mine[g].size() ? mine[g][at] : 0;
      msgs[g] = std::string("internal error: ") + e.what();
    }
  });
  int first = -1;
  for (int g = 0; g < ngpu; g++)
    if (!msgs[g].empty() && (first < 0 || bad[g] < bad[first])) first = g;
  if (first >= 0) fail(msgs[first]);
  std::string body;
  {
    size_t total = 0;
    for (int g = 0; g < ngpu; g++) total += bodies[g].size();
    body.reserve(total);
    std::vector<size_t> next(ngpu, 0), pos(ngpu, 0);
    for (size_t i = 0; i < n; i++) {
      const int g = (int)(fnv1a64(pin.recs[i].target_name) % (uint64_t)ngpu);
      const uint64_t sz = sizes[g][next[g]++];
      body.append(bodies[g], pos[g], sz);
      pos[g] += sz;
    }
  }
  out.write(vcf_header(sample, {}));
  out.write(body);
  out.close();
  return leave(0);
}

int cmd_call_paf(const std::string* input, const std::string& t_fa, const std::string& q_fa, bool snp,
                 uint64_t svlen, const std::string& sample, Output& out) {
  if (g_gpus > 1) return cmd_call_paf_multi(input, t_fa, q_fa, snp, svlen, sample, out, g_gpus);
  Dev d;
  PafInput pin = load_paf(d, input, false);
  DevFasta tf, qf;
  d.init();
  tf.load(d, t_fa);
  qf.load(d, q_fa);
  std::string body;
  size_t bad_at = 0;
  call_paf_run(d, tf, qf, pin, nullptr, pin.recs.size(), nullptr, snp, svlen, body, nullptr, &bad_at);
  /* everything is buffered; the header goes out first, after all records were processed (:294-299) */
  out.write(vcf_header(sample, {}));
  out.write(body);
  out.close();
  return leave(0);
}

/* The reference compiles --query-regex with the Rust `regex` crate (cli.rs:332-343); this host has std::regex (ECMAScript).
 * The two agree on what query names are matched with in practice — literals, classes, `\d \w \s \b`, POSIX classes,
 * repetition (greedy and lazy), alternation, non-capturing groups — and differ at the edges, which are mapped or refused here
 * instead of being left to mean something else: `(?i)` in front (the only inline flag taken) becomes the icase option; named
 * groups `(?P<n>..)` / `(?<n>..)` become plain groups; `\A` / `\z` become `^` / `$`; `\x{HH}` becomes `\xHH`; what the
 * crate rejects at parse time (look-around, back-references) and what std::regex cannot express (other inline flags, Unicode
 * classes `\p{..}`) end the run with the kind of message clap prints for a bad value [approximate text: unpinned]. */
std::string rust_regex_to_ecma(const std::string& pat, bool* icase) {
  auto bad = [&](const char* why) {
    fail(std::string("invalid value '") + pat + "' for '--query-regex <QUERY_REGEX>': regex parse error: " + why);
  };
  std::string out;
  size_t i = 0;
  bool in_class = false;
  while (i < pat.size()) {
    const char c = pat[i];
    if (c == '\\') {
      if (i + 1 >= pat.size()) bad("incomplete escape sequence, reached end of pattern prematurely");
      const char e = pat[i + 1];
      if (e >= '1' && e <= '9') bad("backreferences are not supported");
      if (e == 'p' || e == 'P') bad("Unicode classes are not supported by this build");
      if (e == 'A' && !in_class) {
        out += '^';
      } else if (e == 'z' && !in_class) {
        out += '$';
      } else if (e == 'x' && i + 2 < pat.size() && pat[i + 2] == '{') {
        const size_t close = pat.find('}', i + 3);
        if (close == std::string::npos || close - (i + 3) < 1 || close - (i + 3) > 2) bad("hexadecimal escapes beyond \\x{FF} are not supported by this build");
        std::string hex = pat.substr(i + 3, close - (i + 3));
        if (hex.size() == 1) hex.insert(hex.begin(), '0');
        out += "\\x" + hex;
        i = close + 1;
        continue;
      } else {
        out += c;
        out += e;
      }
      i += 2;
      continue;
    }
    if (in_class) {
      /* what the crate's classes have and ECMAScript's have not is refused, not left to match another set of names: nested
       * classes `[a[bc]]`, intersection / difference / symmetric difference (`&&`, `--`, `~~`); a POSIX class `[:alpha:]`
       * (also negated, `[:^alpha:]`) is one unit — its `]` does not end the class around it */
      if (c == '[') {
        if (i + 1 < pat.size() && pat[i + 1] == ':') {
          const size_t close = pat.find(":]", i + 2);
          if (close == std::string::npos) bad("unclosed POSIX character class");
          if (pat[i + 2] == '^') bad("negated POSIX classes [[:^name:]] are not supported by this build");
          out.append(pat, i, close + 2 - i);
          i = close + 2;
          continue;
        }
        bad("nested character classes are not supported by this build");
      }
      if (i + 1 < pat.size() && (c == '&' || c == '-' || c == '~') && pat[i + 1] == c && (c != '-' || (i + 2 < pat.size() && pat[i + 2] == '[')))
        bad("character class set operations (&&, --, ~~) are not supported by this build");
      if (c == ']') in_class = false;
      out += c;
      i++;
      continue;
    }
    if (c == '[') {
      in_class = true;
      out += c;
      i++;
      if (i < pat.size() && pat[i] == '^') out += pat[i++];
      if (i < pat.size() && pat[i] == ']') out += "\\]", i++; /* a leading ] is a literal in both */
      continue;
    }
    if (c == '(' && i + 1 < pat.size() && pat[i + 1] == '?') {
      const std::string rest = pat.substr(i + 2, 3);
      if (rest.compare(0, 1, ":") == 0) {
        out += "(?:";
        i += 3;
      } else if (rest.compare(0, 2, "P<") == 0 || (rest.compare(0, 1, "<") == 0 && rest.compare(0, 2, "<=") != 0 && rest.compare(0, 2, "<!") != 0)) {
        const size_t close = pat.find('>', i + 2);
        if (close == std::string::npos) bad("unclosed capture group name");
        out += '(';
        i = close + 1;
      } else if (rest.compare(0, 1, "=") == 0 || rest.compare(0, 1, "!") == 0 || rest.compare(0, 2, "<=") == 0 || rest.compare(0, 2, "<!") == 0) {
        bad("look-around, including look-ahead and look-behind, is not supported");
      } else if (rest.compare(0, 2, "i)") == 0 && (i == 0 || (i == 1 && pat[0] == '^'))) {
        *icase = true;
        i += 4;
      } else {
        bad("inline flags other than a leading (?i) are not supported by this build");
      }
      continue;
    }
    out += c;
    i++;
  }
  return out;
}

int cmd_call_maf(const std::string* input, bool snp, bool inv, uint64_t svlen, const std::string& sample,
                 const std::string* query_name, const std::string* query_regex, uint64_t chunk_size, Output& out) {
  Dev d;
  MafDevices md(d);
  MafChunks chunks(input);
  /* utils.rs:414-436: `<input>.index` (JSON written by `maf-index`) supplies ##contig lines */
  std::vector<std::pair<std::string, uint64_t>> contigs;
  if (input) contigs = maf_index_ref_contigs(*input + ".index");
  std::string text = vcf_header(sample, contigs);
  std::regex re;
  if (!query_name && query_regex) { /* cli.rs:332-343 anchors the pattern; maf.rs:267-271 searches from 0 */
    std::string pat = *query_regex;
    if (pat.empty() || pat.front() != '^') pat.insert(pat.begin(), '^');
    if (pat.back() != '$') pat.push_back('$');
    bool icase = false;
    const std::string ecma = rust_regex_to_ecma(pat, &icase);
    try {
      re = std::regex(ecma, icase ? std::regex::ECMAScript | std::regex::icase : std::regex::ECMAScript);
    } catch (std::regex_error& e) {
      fail(std::string("invalid value '") + *query_regex + "' for '--query-regex <QUERY_REGEX>': regex parse error (" + e.what() + ")");
    }
  }
  if (chunk_size == 0) fail("chunk size must be positive (the reference would never terminate)");
  MafInput min;
  /* One device: a piece's rows leave — copy-out and write, 0.07 s per 280 MB — on a helper thread with a context of its own while
   * the next piece is read, uploaded, split and walked (0.43 of a 1.56 s command at configs[2]'s size was this copy-out, in
   * line).  The text buffer is the helper context's; the main thread waits for the helper before it asks for the next one. */
  std::unique_ptr<Dev> dw;
  struct Writer {
    std::thread th;
    std::string err;
    void* text = nullptr;
    void join() {
      if (th.joinable()) th.join();
    }
    ~Writer() { join(); }
  } writer;
  auto writer_done = [&]() { /* the piece in front is out (or failed: its message is raised here, on the command's thread) */
    writer.join();
    if (writer.text) {
      dw->release(writer.text);
      writer.text = nullptr;
    }
    if (!writer.err.empty()) fail(writer.err);
  };
  g_timer.mark("host");
  while (chunks.next(d, min)) { /* one piece of the file at a time, rows written as they are called (caller.rs:62-149) */
  g_timer.mark("read + upload + split");
  std::vector<MafRecord>& all = min.recs;
  /* record selection (:62-108): single-s-line blocks and blocks without the asked query are skipped */
  std::vector<const MafRecord*> recs;
  for (auto& r : all) {
    if (r.slines.size() == 1) continue;
    if (query_name) {
      size_t k = 0;
      for (; k < r.slines.size(); k++)
        if (r.slines[k].name == *query_name) break;
      if (k == r.slines.size()) continue;
      r.query_idx = k;
    } else if (query_regex) {
      size_t k = 0;
      for (; k < r.slines.size(); k++)
        if (std::regex_search(r.slines[k].name, re)) break;
      if (k == r.slines.size()) continue;
      r.query_idx = k;
    } else {
      r.query_idx = 1;
    }
    if (r.q().seq_size() < r.t().seq_size())
      fail("panic: query row shorter than the target row (caller.rs:175 slice out of range)");
    recs.push_back(&r);
  }
  const uint32_t n = (uint32_t)recs.size();
  if (n) {
    /* every device walks its range of the blocks (K4: count, scan, fill) and turns the run list into rows where it lies (K19:
     * count, scan, fill); only text comes back, in block order */
    struct Part {
      const uint8_t* d_text = nullptr;
      uint64_t n_text = 0;
      uint32_t lo = 0, bad = UINT32_MAX; /* first block of the range; the range's first failing block (range-relative) */
      wga_vcf_err err{};
    };
    std::vector<Part> parts(md.count());
    md.run(min, recs, true /* total_size = target row length (:115) */, [&](int g, Dev& dg, const MafRows& p, uint32_t lo, uint32_t cnt) {
      auto* d_cnt = (uint64_t*)dg.alloc((size_t)cnt * 8);
      dg.check(wga_maf_call_runs(dg.ctx, cnt, p.d_rows, p.d_t, p.d_q, p.d_c, d_cnt, nullptr, nullptr));
      uint64_t n_runs = 0;
      uint64_t* d_roff = dg.scan(cnt, d_cnt, &n_runs);
      auto* d_runs = (uint64_t*)dg.alloc((3 * n_runs + 3) * 8);
      dg.check(wga_maf_call_runs(dg.ctx, cnt, p.d_rows, p.d_t, p.d_q, p.d_c, d_cnt, d_runs, d_roff));
      /* names (each once) and the s lines' fields go up */
      std::string names;
      std::unordered_map<std::string, uint64_t> name_at;
      auto name_off = [&](const std::string& nm) {
        auto it = name_at.find(nm);
        if (it != name_at.end()) return it->second;
        const uint64_t at = names.size();
        names += nm;
        name_at.emplace(nm, at);
        return at;
      };
      std::vector<wga_maf_vcf_rec> vr(cnt);
      for (uint32_t k = 0; k < cnt; k++) {
        const MafRecord& r = *recs[lo + k];
        wga_maf_vcf_rec& v = vr[k];
        v.t_name_off = name_off(r.t().name), v.t_name_len = (uint32_t)r.t().name.size();
        v.q_name_off = name_off(r.q().name), v.q_name_len = (uint32_t)r.q().name.size();
        v.t_start = r.t().start, v.q_start = r.q().start, v.q_size = r.q().size;
        v.q_neg = r.q().neg ? 1u : 0u, v.pad = 0;
      }
      names.push_back('\0'); /* never empty */
      const uint8_t* d_names = dg.upload((const uint8_t*)names.data(), names.size());
      const wga_maf_vcf_rec* d_vr = dg.upload(vr.data(), vr.size());
      auto* d_nb = (uint64_t*)dg.alloc((size_t)cnt * 8);
      auto* d_err = (wga_vcf_err*)dg.alloc((size_t)cnt * sizeof(wga_vcf_err));
      dg.check(wga_maf_call_vcf(dg.ctx, cnt, p.d_rows, p.d_t, p.d_q, p.d_c, d_runs, d_roff, d_vr, d_names, snp, inv, svlen, chunk_size,
                                d_nb, d_err, nullptr, nullptr));
      auto* d_toff = (uint64_t*)dg.alloc(((size_t)cnt + 1) * 8);
      dg.check(wga_exclusive_scan_u64(dg.ctx, cnt, d_nb, d_toff));
      std::vector<wga_vcf_err> errs(cnt);
      dg.download(errs.data(), (const wga_vcf_err*)d_err, cnt);
      Part& pt = parts[g];
      pt.lo = lo;
      uint32_t upto = cnt; /* blocks whose text is written: all, or up to and with the first failing one (its chunks in front of the failing one) */
      for (uint32_t k = 0; k < cnt; k++)
        if (errs[k].item != WGA_NONE) {
          pt.bad = k, pt.err = errs[k];
          upto = k + 1;
          break;
        }
      dg.download(&pt.n_text, (const uint64_t*)d_toff + upto, 1);
      if (pt.n_text) {
        uint8_t* d_text;
        if (md.count() == 1) { /* the helper's buffer: the piece in front must be out before its memory is asked for again */
          if (!dw) {
            dw.reset(new Dev());
            dw->helper = true;
            dw->init();
          }
          writer_done();
          d_text = (uint8_t*)dw->alloc(pt.n_text + 64);
        } else {
          d_text = (uint8_t*)dg.alloc(pt.n_text + 64);
        }
        dg.check(wga_maf_call_vcf(dg.ctx, upto, p.d_rows, p.d_t, p.d_q, p.d_c, d_runs, d_roff, d_vr, d_names, snp, inv, svlen,
                                  chunk_size, nullptr, nullptr, d_text, d_toff));
        pt.d_text = d_text;
      }
    });
    g_timer.mark("kernels (runs, rules, VCF text)");
    /* the ranges' texts leave in block order, up to the first range that holds a failing block (its rows in front of the
     * failing chunk are written, then the error is raised: caller.rs:137-141) */
    if (md.count() == 1) writer_done();
    out.write(text);
    text.clear();
    for (int g = 0; g < md.count(); g++) {
      Part& pt = parts[g];
      if (pt.n_text) {
        if (md.count() == 1 && pt.bad == UINT32_MAX) { /* off it goes; the main thread turns to the next piece */
          md.dev(0).check(wga_sync(md.dev(0).ctx)); /* the rows are written */
          writer.text = (void*)pt.d_text;
          const uint8_t* src = pt.d_text;
          const uint64_t nbytes = pt.n_text;
          writer.th = std::thread([&, src, nbytes] {
            try {
              stream_out(*dw, out, src, (size_t)nbytes, false);
            } catch (Error& e) {
              writer.err = e.msg.empty() ? std::string("error") : e.msg;
            } catch (std::exception& e) {
              writer.err = std::string("internal error: ") + e.what();
            }
          });
        } else {
          if (md.count() == 1) md.dev(0).check(wga_sync(md.dev(0).ctx));
          stream_out(md.count() == 1 ? *dw : md.dev(g), out, pt.d_text, pt.n_text);
          if (md.count() == 1) dw->release((void*)pt.d_text);
        }
      }
      if (pt.bad != UINT32_MAX)
        fail(std::string("invalid reference/alternate base `") + (char)pt.err.ch + "` for a VCF record (noodles-vcf parse error)");
    }
    g_timer.mark("copy-out + write");
  }
  md.release_all();
  }
  writer_done();
  out.write(text);
  out.close();
  return leave(0);
}
