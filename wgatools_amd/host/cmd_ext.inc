/* cmd_ext.inc — part of wgatools_main.cpp (included there, inside its namespace: the commands share the device helpers, readers and
 * writers defined in front of the include). */
/* ---- maf-index (tools/index.rs:14-94, utils.rs:334-350) ----------------------------------------------------------------------
 * The blocks come from the piece reader and the device splitter (MafChunks); a block's file offset is the position behind the
 * line that ended the record in front of it (index.rs:22 takes the stream position in front of every records().next(), which
 * has consumed that line: maf.rs:409-411), behind the header line for the first block.  The offsets are found by a walk over
 * the piece's line starts that keeps its state across pieces; a piece's bytes behind its "#\n" prefix are consecutive bytes
 * of the file (the `pending` tail of a piece opens the next one), so the file position of a piece is the sum of the pieces in
 * front of it. */
struct MafOffsetWalk {
  uint64_t file_pos = 0; /* of the piece's first byte behind its prefix */
  uint64_t cur = 0;      /* behind the last line that ended a record */
  bool in_run = false, first_line = true, first_piece = true;
  void piece(const std::string& text, std::vector<uint64_t>& offsets) {
    const size_t skip = first_piece ? 0 : 2;
    first_piece = false;
    size_t p = skip;
    while (p < text.size()) {
      const void* nl = memchr(text.data() + p, '\n', text.size() - p);
      const size_t end = nl ? (size_t)((const char*)nl - text.data()) + 1 : text.size();
      if (first_line) { /* the header, whatever it starts with (maf.rs:25-36) */
        first_line = false;
        cur = file_pos + (end - skip);
      } else if (text[p] == 's') {
        if (!in_run) offsets.push_back(cur);
        in_run = true;
      } else if (in_run) {
        in_run = false;
        cur = file_pos + (end - skip);
      }
      p = end;
    }
    file_pos += text.size() - skip;
  }
};

int cmd_maf_index(const std::string* input, const std::string& outfile) {
  if (!input || *input == "-") fail("the following required arguments were not provided: <INPUT>");
  { /* the reference reads the file as it is (MAFReader<File>) and maf-ext reads blocks at the index's offsets with pread: a
     * compressed file cannot be indexed, and the piece reader would inflate it and index the inflated stream */
    FILE* f = fopen(input->c_str(), "rb");
    if (!f) fail(*input + ": " + strerror(errno));
    unsigned char magic[2] = {0, 0};
    const size_t got = fread(magic, 1, 2, f);
    fclose(f);
    if (got == 2 && magic[0] == 0x1f && magic[1] == 0x8b)
      fail("maf-index reads the file as it is: `" + *input + "` is gzip / BGZF compressed, index the plain file");
  }
  Dev d;
  MafChunks chunks(input); /* index.rs / utils.rs:346: the input is opened first */
  Output out;
  out.open(outfile == "-" ? *input + ".index" : outfile, true); /* utils.rs:336-348: always overwritten */
  struct Entry {
    std::string name;
    std::string ivls;
    uint64_t size;
    bool isref;
  };
  std::vector<Entry> entries;
  std::unordered_map<std::string, size_t> by_name;
  MafOffsetWalk walk;
  MafInput min;
  std::vector<uint64_t> offsets;
  static const char* kConflict = "Same sequence cannot be both reference and query!";
  /* WGA_MAF_INDEX_WRITER=host: every piece through the host loop below, as before K35.  Otherwise a piece the device splitter took
   * goes through wga_maf_index: no record is built and no second walk over its text runs for it; the offset walk runs only over the
   * pieces the host reader reads and hands its state to the device pieces and takes it back. */
  const bool host_writer = env_is("WGA_MAF_INDEX_WRITER", "host");
  chunks.lines_only = !host_writer;
  if (host_writer) chunks.on_piece = [&](const std::string& text) { walk.piece(text, offsets); }; /* pieces without a block are walked too */
  for (;;) {
    offsets.clear();
    if (!chunks.next(d, min)) break;
    if (!host_writer && min.d_lines) {
      const uint32_t skip = walk.first_piece ? 0u : 2u;
      const size_t n_bytes = min.text->size();
      void* d_work = d.alloc((size_t)wga_maf_index_work_bytes(min.n_lines));
      uint64_t n_names = 0, n_blocks = 0, n_slines = 0, text_bytes = 0, dup = WGA_NONE, conflict = WGA_NONE, next_offset = walk.cur;
      auto call = [&](wga_maf_index_name* d_names, uint8_t* d_out) {
        return wga_maf_index(d.ctx, min.d_text, n_bytes, min.d_lines, min.n_lines, skip, walk.file_pos, walk.cur, d_work, &n_names,
                             &n_blocks, &n_slines, &text_bytes, &dup, &conflict, &next_offset, d_names, d_out);
      };
      const int rc = call(nullptr, nullptr);
      if (rc != WGA_E_FALLBACK) {
        d.check(rc);
        std::vector<wga_maf_index_name> names((size_t)n_names + 1);
        std::string ivl_text((size_t)text_bytes, '\0');
        if (n_slines) {
          auto* d_names = (wga_maf_index_name*)d.alloc(names.size() * sizeof(wga_maf_index_name));
          auto* d_out = (uint8_t*)d.alloc((size_t)text_bytes + 16);
          d.check(call(d_names, d_out));
          d.download(names.data(), d_names, names.size());
          d.download((uint8_t*)&ivl_text[0], d_out, (size_t)text_bytes);
        }
        /* the piece's names -> the global entries: one lookup per distinct name of the piece.  The error is the one at the lowest
         * line: the device's two, or the first line of a group whose isref is not its entry's; a duplicate goes first on the same
         * line (index.rs:32-56) */
        const std::string& text = *min.text;
        std::vector<size_t> entry_of((size_t)n_names);
        for (size_t g = 0; g < (size_t)n_names; g++) {
          const wga_maf_index_name& N = names[g];
          std::string name(text, (size_t)N.name_off, N.name_len);
          auto it = by_name.find(name);
          if (it == by_name.end()) {
            it = by_name.emplace(name, entries.size()).first;
            entries.push_back(Entry{std::move(name), std::string(), N.size, N.isref != 0});
          } else if (entries[it->second].isref != (N.isref != 0)) {
            conflict = std::min(conflict, N.first_line);
          }
          entry_of[g] = it->second;
        }
        if (dup != WGA_NONE && dup <= conflict) {
          wga_maf_line L;
          d.download(&L, (const wga_maf_line*)min.d_lines + dup, 1);
          fail("Duplicate name `" + std::string(text, (size_t)L.name_off, L.name_len) + "` in a record not allowed, please check or use `rename`");
        }
        if (conflict != WGA_NONE) fail(kConflict);
        for (size_t g = 0; g < (size_t)n_names; g++) {
          std::string& v = entries[entry_of[g]].ivls;
          if (!v.empty()) v.push_back(',');
          v.append(ivl_text, (size_t)names[g].text_off, (size_t)(names[g + 1].text_off - names[g].text_off));
        }
        walk.file_pos += n_bytes - skip;
        walk.cur = next_offset;
        walk.first_piece = walk.first_line = walk.in_run = false;
        d.release_all();
        g_timer.mark("maf-index entries (device)");
        continue;
      }
      min.recs = parse_maf(*min.text, &min.header); /* a line the splitter does not take: the host reader's records, or its error */
    }
    if (!host_writer) walk.piece(*min.text, offsets);
    if (offsets.size() != min.recs.size()) fail("internal error: maf-index lost track of the blocks' offsets");
    for (size_t b = 0; b < min.recs.size(); b++) {
      const MafRecord& r = min.recs[b];
      for (size_t i = 0; i < r.slines.size(); i++) {
        const MafSLine& s = r.slines[i];
        for (size_t k = 0; k < i; k++)
          if (r.slines[k].name == s.name)
            fail("Duplicate name `" + s.name + "` in a record not allowed, please check or use `rename`");
        auto it = by_name.find(s.name);
        if (it == by_name.end()) {
          it = by_name.emplace(s.name, entries.size()).first;
          entries.push_back(Entry{s.name, std::string(), s.size, i == 0});
        } else if (entries[it->second].isref != (i == 0)) {
          fail("Same sequence cannot be both reference and query!");
        }
        std::string& v = entries[it->second].ivls;
        if (!v.empty()) v.push_back(',');
        v += "{\"start\":";
        append_u64(v, s.start);
        v += ",\"end\":";
        append_u64(v, s.start + s.align_size);
        v += s.neg ? ",\"strand\":\"-\",\"offset\":" : ",\"strand\":\"+\",\"offset\":";
        append_u64(v, offsets[b]);
        v.push_back('}');
      }
    }
    if (d.ctx) d.release_all();
    g_timer.mark("maf-index entries (host)");
  }
  if (entries.empty()) fail("Empty record");
  std::string js = "{";
  for (size_t e = 0; e < entries.size(); e++) {
    if (e) js.push_back(',');
    append_json_string(js, entries[e].name);
    js += ":{\"ivls\":[" + entries[e].ivls + "],\"size\":";
    append_u64(js, entries[e].size);
    js += entries[e].isref ? ",\"isref\":true}" : ",\"isref\":false}";
  }
  js.push_back('}');
  out.write(js);
  out.close();
  return leave(0);
}

/* ---- maf-ext (tools/mafextra.rs, utils.rs:353-394) ----------------------------------------------------------------------------
 * The regions' hits are looked up in per-name interval arrays sorted once (rust-lapper's find: iv.start < g_end && iv.end >
 * g_start, in the order of a stable sort by (start, end)); only the blocks that are hit are read (pread; a block's span ends
 * at the next larger offset of the index or at the end of the file).  The hits are written in WINDOWS of consecutive hits: a
 * window's distinct blocks are gathered into one piece, split on the device and cut by K21 (wga_maf_slice). */
struct ExtRegion {
  std::string name;
  uint64_t start, end;
};
struct ExtHit {
  size_t region;
  uint64_t offset, b_start, b_end;
};
static const char* kExtShortRow = "panic: a row is shorter than the slice's end (maf.rs:240 slice index out of range)";

static ExtRegion ext_region_checked(const std::string& name, uint64_t s, uint64_t e) {
  if (s > e)
    fail("Parse Genome Region Error By: Start `" + std::to_string(s) + "` is larger than end `" + std::to_string(e) + "`");
  return ExtRegion{name, s, e};
}
static bool ext_u64(const std::string& t, uint64_t* v) {
  if (t.empty() || t.find_first_not_of("0123456789") != std::string::npos) return false;
  errno = 0;
  *v = strtoull(t.c_str(), nullptr, 10);
  return errno != ERANGE;
}
static ExtRegion ext_parse_region(const std::string& r) { /* mafextra.rs:79-113 */
  static const std::regex re("^([a-zA-Z0-9.@_#-]+):([0-9]+)-([0-9]+)$");
  std::smatch m;
  uint64_t s = 0, e = 0;
  if (!std::regex_match(r, m, re) || !ext_u64(m[2].str(), &s) || !ext_u64(m[3].str(), &e))
    fail("Parse Genome Region Error By: Region `" + r + "` is match the format of `chr:start-end`");
  return ext_region_checked(m[1].str(), s, e);
}

/* the reference's slice on the host for rows with non-ASCII text: get_col_coord counts characters and its result is used as a
 * byte index (maf.rs:81-95, 232-234); a cut inside a character panics */
static uint64_t ext_host_col(const MafSLine& s, uint64_t pos) {
  uint64_t chars = 0, bases = 0;
  for (size_t i = 0; i < s.seq_size(); i++) {
    const unsigned char ch = (unsigned char)s.seq_data()[i];
    if ((ch & 0xC0u) == 0x80u) continue;
    if (ch != '-') {
      if (bases == pos) return chars;
      bases++;
    }
    chars++;
  }
  return s.seq_size();
}
static void ext_write_row(std::string& t, const MafSLine& s, uint64_t start, uint64_t size, const char* seq, size_t n) {
  t += "s\t" + s.name + "\t" + std::to_string(start) + "\t" + std::to_string(size) + (s.neg ? "\t-\t" : "\t+\t") +
       std::to_string(s.size) + "\t";
  t.append(seq, n);
  t += "\n";
}
static bool ext_host_slice(const MafRecord& r, size_t ord, uint64_t cut_lo, uint64_t cut_hi, std::string& t, std::string& panic) {
  const uint64_t c0 = ext_host_col(r.slines[ord], cut_lo), c1 = ext_host_col(r.slines[ord], cut_hi);
  std::string rec = "a score=255\n";
  for (size_t i = 0; i < r.slines.size(); i++) {
    const MafSLine& s = r.slines[i];
    if (c0 > c1 || s.seq_size() < c1) {
      panic = kExtShortRow;
      return false;
    }
    for (uint64_t x : {c0, c1})
      if (x < s.seq_size() && ((unsigned char)s.seq_data()[x] & 0xC0u) == 0x80u) {
        panic = "panic: a cut falls inside a character (maf.rs:234 byte index is not a char boundary)";
        return false;
      }
    uint64_t gaps = 0;
    for (uint64_t x = c0; x < c1; x++) gaps += s.seq_data()[x] == '-';
    ext_write_row(rec, s, s.start + cut_lo, i == ord ? cut_hi - cut_lo : (c1 - c0) - gaps, s.seq_data() + c0, (size_t)(c1 - c0));
  }
  t += rec + "\n";
  return true;
}

int cmd_maf_ext(const std::string* input, const std::vector<std::string>* region_list, const std::string* region_file,
                const std::string& outfile, bool rewrite) {
  if (!region_list && !region_file) fail("regions or region_file must be specified"); /* utils.rs:361-363 */
  Output out;
  out.open(outfile, rewrite);
  if (!input || *input == "-") fail("Stdin not allowed here");
  const int fd = open(input->c_str(), O_RDONLY);
  if (fd < 0) fail(*input + ": " + strerror(errno));
  struct FdGuard {
    int fd;
    ~FdGuard() { close(fd); }
  } guard{fd};
  struct stat st;
  if (fstat(fd, &st) != 0) fail(*input + ": " + strerror(errno));
  const uint64_t file_size = (uint64_t)st.st_size;
  const std::string index_path = *input + ".index";
  {
    FILE* f = fopen(index_path.c_str(), "rb");
    if (!f) fail(index_path + ": " + strerror(errno));
    fclose(f);
  }
  std::vector<MafIndexItem> index = parse_maf_index(read_all(&index_path), true);
  /* mafextra.rs:41-67: the -r regions, then the file's */
  std::vector<ExtRegion> regions;
  if (region_list)
    for (const std::string& r : *region_list) regions.push_back(ext_parse_region(r));
  if (region_file) {
    FILE* f = fopen(region_file->c_str(), "rb");
    if (!f) fail(*region_file + ": " + strerror(errno));
    fclose(f);
    const std::string text = read_all(region_file);
    size_t p = 0, line_no = 0;
    while (p < text.size()) {
      size_t e = text.find('\n', p);
      if (e == std::string::npos) e = text.size();
      std::string ln = text.substr(p, e - p);
      p = e + 1;
      line_no++;
      if (!ln.empty() && ln.back() == '\r') ln.pop_back();
      if (ln.empty()) continue;
      const size_t t1 = ln.find('\t'), t2 = t1 == std::string::npos ? t1 : ln.find('\t', t1 + 1);
      uint64_t s = 0, en = 0;
      if (t2 == std::string::npos || ln.find('\t', t2 + 1) != std::string::npos || !ext_u64(ln.substr(t1 + 1, t2 - t1 - 1), &s) ||
          !ext_u64(ln.substr(t2 + 1), &en))
        fail("CSV deserialize error: record " + std::to_string(line_no - 1) + " (line: " + std::to_string(line_no) +
             "): expected name<TAB>start<TAB>end");
      regions.push_back(ext_region_checked(ln.substr(0, t1), s, en));
    }
  }
  out.write("#maf version=1.6 cmd=maf_extract\n"); /* mafextra.rs:33-35 */
  /* per-name interval arrays, sorted once; every offset of the index, sorted: a block's span ends at the next larger one */
  std::unordered_map<std::string, size_t> by_name;
  std::vector<uint64_t> all_offsets;
  std::vector<std::vector<uint64_t>> end_max(index.size());
  for (size_t i = 0; i < index.size(); i++) {
    by_name[index[i].name] = i; /* serde: the last of equal keys stays */
    std::stable_sort(index[i].ivls.begin(), index[i].ivls.end(), [](const MafIndexIvl& a, const MafIndexIvl& b) {
      return a.start != b.start ? a.start < b.start : a.end < b.end;
    });
    for (const MafIndexIvl& iv : index[i].ivls) all_offsets.push_back(iv.offset);
    /* the running maximum of `end` in that order: the intervals in front of the first one whose maximum passes g_start all
     * end at or before it, so a region's scan starts there (a binary search) instead of at the name's first interval */
    end_max[i].reserve(index[i].ivls.size());
    uint64_t m = 0;
    for (const MafIndexIvl& iv : index[i].ivls) end_max[i].push_back(m = std::max(m, iv.end));
  }
  std::sort(all_offsets.begin(), all_offsets.end());
  all_offsets.erase(std::unique(all_offsets.begin(), all_offsets.end()), all_offsets.end());
  std::vector<ExtHit> hits;
  std::vector<size_t> failed;
  for (size_t r = 0; r < regions.size(); r++) {
    const ExtRegion& g = regions[r];
    auto it = by_name.find(g.name);
    const size_t before = hits.size();
    if (it != by_name.end()) {
      const std::vector<MafIndexIvl>& v = index[it->second].ivls;
      const size_t hi = (size_t)(std::lower_bound(v.begin(), v.end(), g.end, [](const MafIndexIvl& a, uint64_t e) { return a.start < e; }) -
                                 v.begin()); /* the intervals with start < g_end */
      const std::vector<uint64_t>& em = end_max[it->second];
      const size_t lo = (size_t)(std::upper_bound(em.begin(), em.begin() + (ptrdiff_t)hi, g.start) - em.begin());
      for (size_t k = lo; k < hi; k++)
        if (v[k].end > g.start) hits.push_back(ExtHit{r, v[k].offset, v[k].start, v[k].end});
    }
    if (hits.size() == before) failed.push_back(r);
  }
  g_timer.mark("index + regions");
  size_t budget = (size_t)1 << 28, piece_cap = (size_t)1 << 30;
  if (const char* e = getenv("WGA_MAF_EXT_OUT_BYTES")) budget = std::max<size_t>(1, (size_t)strtoull(e, nullptr, 10));
  if (const char* e = getenv("WGA_CHUNK_BYTES")) piece_cap = std::max<size_t>(1, (size_t)strtoull(e, nullptr, 10));
  auto span_of = [&](uint64_t off) -> uint64_t {
    if (off > file_size) fail("the index does not belong to this file: a block's offset lies behind its end");
    auto nx = std::upper_bound(all_offsets.begin(), all_offsets.end(), off);
    return (nx == all_offsets.end() ? file_size : std::min<uint64_t>(*nx, file_size)) - off;
  };
  Dev d;
  MafDevices md(d);
  std::string pending_error;
  for (size_t h0 = 0; h0 < hits.size() && pending_error.empty();) {
    /* the window: hits [h0, h1); a hit's text is bounded by its block's span: the rows' text and names once, and at most 75
     * bytes of fields for each of its lines (an input line holds 13 bytes or more) */
    std::map<uint64_t, size_t> blocks; /* offset -> index among the window's blocks */
    std::vector<uint64_t> block_off;
    uint64_t text_bound = 0, piece_bytes = 2;
    size_t h1 = h0;
    for (; h1 < hits.size(); h1++) {
      const uint64_t span = span_of(hits[h1].offset), tb = 8 * span + 32;
      const bool fresh = !blocks.count(hits[h1].offset);
      if (h1 > h0 && (text_bound + tb > budget || (fresh && piece_bytes + span + 1 > piece_cap))) break;
      if (fresh) {
        blocks.emplace(hits[h1].offset, block_off.size());
        block_off.push_back(hits[h1].offset);
        piece_bytes += span + 1;
      }
      text_bound += tb;
    }
    /* the piece: "#\n" (the reader's header line), then every block's span and a line feed */
    std::string piece = "#\n";
    std::vector<uint64_t> pos(block_off.size());
    piece.reserve((size_t)piece_bytes + 16);
    for (size_t b = 0; b < block_off.size(); b++) {
      const uint64_t span = span_of(block_off[b]);
      pos[b] = piece.size();
      const size_t at = piece.size();
      piece.resize(at + (size_t)span);
      for (uint64_t got = 0; got < span;) {
        const ssize_t k = pread(fd, &piece[at + got], (size_t)(span - got), (off_t)(block_off[b] + got));
        if (k <= 0) fail(*input + ": read error");
        got += (uint64_t)k;
      }
      piece.push_back('\n');
    }
    g_timer.mark("pread blocks");
    /* every block's record: the first one of its span (mafextra.rs:188-190) */
    std::vector<const MafRecord*> rec_of(block_off.size(), nullptr);
    std::vector<std::vector<MafRecord>> host_recs;
    MafInput min = maf_from_text(d, std::move(piece));
    bool non_ascii = false;
    if (min.on_device) {
      for (const MafRecord& r : min.recs) {
        const size_t b = (size_t)(std::upper_bound(pos.begin(), pos.end(), r.slines[0].seq_off) - pos.begin()) - 1;
        if (!rec_of[b]) rec_of[b] = &r;
      }
    } else { /* the host reader keeps no offsets: span by span */
      host_recs.resize(block_off.size());
      for (size_t b = 0; b < block_off.size(); b++) {
        const size_t end = b + 1 < pos.size() ? (size_t)pos[b + 1] : min.text->size();
        std::string hdr;
        host_recs[b] = parse_maf("#\n" + min.text->substr((size_t)pos[b], end - (size_t)pos[b]), &hdr);
        if (!host_recs[b].empty()) rec_of[b] = &host_recs[b][0];
      }
      for (const MafRecord* r : rec_of)
        if (r)
          for (const MafSLine& s : r->slines)
            for (size_t x = 0; x < s.seq_size() && !non_ascii; x++) non_ascii = (unsigned char)s.seq_data()[x] >= 0x80u;
    }
    /* the window's hits -> K21's tables (or the host path; the host reader's path and the non-ASCII test above are the only
     * host loops over row text) */
    std::string host_text;
    std::vector<wga_maf_slice_hit> win; /* row0 is set where the hits' device makes its row table */
    std::vector<size_t> win_block;
    for (size_t h = h0; h < h1; h++) {
      const ExtHit& H = hits[h];
      const ExtRegion& g = regions[H.region];
      const size_t b = blocks[H.offset];
      if (!rec_of[b]) fail("Empty record"); /* mafextra.rs:190 */
      const MafRecord& r = *rec_of[b];
      size_t ord = 0;
      for (; ord < r.slines.size(); ord++)
        if (r.slines[ord].name == g.name) break;
      if (ord == r.slines.size()) continue; /* mafextra.rs:193-196 */
      const bool whole = g.start <= H.b_start && g.end >= H.b_end;
      const uint64_t r_start = std::max(H.b_start, g.start), r_end = std::min(H.b_end, g.end);
      if (!whole && r_start < r.slines[ord].start) fail("the index does not belong to this file: a block starts behind its interval");
      const uint64_t cut_lo = whole ? 0 : r_start - r.slines[ord].start, cut_hi = whole ? 0 : r_end - r.slines[ord].start;
      if (non_ascii) {
        if (whole) {
          host_text += "a score=255\n";
          for (const MafSLine& s : r.slines) ext_write_row(host_text, s, s.start, s.align_size, s.seq_data(), s.seq_size());
          host_text += "\n";
        } else if (!ext_host_slice(r, ord, cut_lo, cut_hi, host_text, pending_error)) {
          break;
        }
        continue;
      }
      win.push_back(wga_maf_slice_hit{0, cut_lo, cut_hi, (uint32_t)r.slines.size(), (uint32_t)ord, whole ? 1u : 0u, 0u});
      win_block.push_back(b);
    }
    /* hits [lo, hi) of the window on one device: their text in HBM, its length and the first short hit */
    struct Part {
      const uint8_t* text = nullptr;
      uint64_t bytes = 0;
      uint32_t first_short = 0xFFFFFFFFu;
    };
    /* The in-place table names the rows of all the window's blocks where the piece was uploaded (device 0, device splitter);
     * every other device, and the host reader's records, get a gathered copy of the rows their hits name. */
    auto run_part = [&](Dev& dg, bool in_place, size_t lo, size_t hi) {
      Part p;
      dg.init();
      std::vector<wga_maf_slice_hit> part(win.begin() + (ptrdiff_t)lo, win.begin() + (ptrdiff_t)hi);
      std::vector<const MafRecord*> recs = rec_of;
      std::vector<size_t> slot(win_block.begin() + (ptrdiff_t)lo, win_block.begin() + (ptrdiff_t)hi); /* a hit's block in recs */
      if (!in_place) {
        std::unordered_map<size_t, size_t> seen;
        recs.clear();
        for (size_t& b : slot) {
          auto it = seen.find(b);
          if (it == seen.end()) {
            it = seen.emplace(b, recs.size()).first;
            recs.push_back(rec_of[b]);
          }
          b = it->second;
        }
      }
      const MafRowTable<wga_maf_slice_row> t = maf_row_table<wga_maf_slice_row>(dg, min, in_place, recs.data(), recs.size());
      uint64_t lines = 0;
      for (size_t k = 0; k < part.size(); k++) {
        part[k].row0 = t.row0[slot[k]];
        lines += part[k].n_rows;
      }
      auto* d_hits = dg.upload(part);
      const uint32_t nh = (uint32_t)part.size();
      maf_window_call(dg, (size_t)wga_maf_slice_work_bytes(nh, lines, t.rows.size(), t.n_cols), d_hits,
                      [&](void* d_work, uint64_t* bytes, uint8_t* d_out) {
                        return wga_maf_slice(dg.ctx, t.d_text, t.d_rows, t.rows.size(), t.n_cols, nh, d_hits, lines, d_work, bytes,
                                             &p.first_short, d_out);
                      },
                      [&](Dev&, const uint8_t* text, size_t bytes) {
                        p.text = text;
                        p.bytes = bytes;
                      });
      return p;
    };
    if (non_ascii) {
      out.write(host_text);
    } else if (!win.empty()) {
      /* --gpus N: device g takes a contiguous range of the window's hits; the texts leave in device order and end behind the
       * first device that met a short row */
      const int ng = (int)std::min<size_t>((size_t)md.count(), win.size());
      std::vector<Part> parts((size_t)ng);
      if (ng == 1) {
        parts[0] = run_part(d, min.on_device, 0, win.size());
      } else {
        on_devices(ng, [&](int g) {
          parts[(size_t)g] = run_part(md.dev(g), g == 0 && min.on_device, win.size() * (size_t)g / (size_t)ng,
                                      win.size() * (size_t)(g + 1) / (size_t)ng);
        });
      }
      for (int g = 0; g < ng && pending_error.empty(); g++) {
        stream_out(md.dev(g), out, parts[(size_t)g].text, (size_t)parts[(size_t)g].bytes);
        if (parts[(size_t)g].first_short != 0xFFFFFFFFu) pending_error = kExtShortRow;
      }
    }
    md.release_all();
    h0 = h1;
  }
  out.close();
  g_timer.mark("write");
  if (!pending_error.empty()) fail(pending_error);
  for (size_t r : failed) /* utils.rs:384-387 */
    log_warn("Failed region: " + regions[r].name + ":" + std::to_string(regions[r].start) + "-" + std::to_string(regions[r].end));
  return leave(0);
}
