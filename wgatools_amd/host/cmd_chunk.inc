/* cmd_chunk.inc — part of wgatools_main.cpp (included there, inside its namespace: the commands share the device helpers, readers and
 * writers defined in front of the include). */
/* ---- chunk (chunk.rs:20-90, utils.rs:656-677) ------------------------------------------------------------------------------
 * Every block is cut into records of at most L columns of its first row; K20 (wga_maf_chunk) counts, places and writes them on
 * the device where the rows were uploaded.  A piece's records are written in WINDOWS of bounded text (WGA_MAF_CHUNK_OUT_BYTES,
 * 256 MiB): `-l 1` turns a 1 GiB piece into ~40 GB.  The windows are planned from an upper bound of a record's text (name,
 * three 20-digit numbers and the slice width per row); a record above the budget is a window of its own. */
static uint64_t chunk_count(uint64_t bl, uint64_t L) { return bl == 0 ? 1 : (bl - 1) / L + 1; } /* chunk.rs:43-56 */

/* the reference builds a record whole before it writes it (chunk.rs:48-49): a row shorter than a chunk's end panics there and
 * the records in front of that chunk are the output */
static const char* kChunkShortRow = "panic: a row is shorter than the block's first row (chunk.rs:75 slice index out of range)";

/* chunk k of every block in [0, n) that is written: kc[b] records of block b (all of them, or the ones in front of a short
 * row's panic); returns the number of blocks that take part (the panic's block included) */
static uint32_t chunk_plan(const MafRecord* const* recs, uint32_t n, uint64_t L, std::vector<uint64_t>& kc, bool* panic) {
  kc.assign(n, 0);
  *panic = false;
  for (uint32_t b = 0; b < n; b++) {
    const MafRecord& r = *recs[b];
    const uint64_t bl = r.slines[0].seq_size(), nk = chunk_count(bl, L);
    uint64_t cut = nk;
    for (const MafSLine& s : r.slines)
      if (s.seq_size() < bl) cut = std::min<uint64_t>(cut, s.seq_size() / L); /* the first chunk whose end passes the row's */
    kc[b] = cut;
    if (cut < nk) {
      *panic = true;
      return b + 1;
    }
  }
  return n;
}

/* the records of blocks recs[0 .. n) (kc[b] chunks each) on device d, window by window */
static void chunk_blocks(Dev& d, const MafInput& in, bool in_place, const MafRecord* const* recs, uint32_t n, const uint64_t* kc,
                         uint64_t L, size_t budget, const MafSink& sink) {
  d.init();
  const MafRowTable<wga_maf_chunk_row> t = maf_row_table<wga_maf_chunk_row>(d, in, in_place, recs, n);
  std::vector<uint64_t> bound(n); /* of a record's text: name, three 20-digit numbers and the slice width per row */
  for (uint32_t b = 0; b < n; b++) {
    const uint64_t w = std::min<uint64_t>(L, recs[b]->slines[0].seq_size());
    bound[b] = 13;
    for (const MafSLine& s : recs[b]->slines) bound[b] += s.name.size() + 70u + w;
  }
  auto* d_carry = (uint64_t*)d.alloc(std::max<size_t>(t.rows.size(), 1) * 8);
  d.check(wga_memset(d.ctx, d_carry, 0, std::max<size_t>(t.rows.size(), 1) * 8));
  g_timer.mark("host rows + upload");
  std::vector<wga_maf_chunk_block> win;
  uint64_t used = 0, lines = 0;
  auto flush = [&]() {
    if (win.empty()) return;
    auto* d_blocks = d.upload(win);
    const uint32_t nb = (uint32_t)win.size();
    maf_window_call(d, (size_t)wga_maf_chunk_work_bytes(nb, lines), d_blocks, [&](void* d_work, uint64_t* bytes, uint8_t* d_out) {
      return wga_maf_chunk(d.ctx, t.d_text, t.d_rows, nb, d_blocks, lines, L, d_carry, d_work, bytes, d_out);
    }, sink);
    win.clear();
    used = lines = 0;
  };
  const uint64_t max_lines = (uint64_t)1 << 31;
  for (uint32_t b = 0; b < n; b++) {
    const uint32_t nr = (uint32_t)recs[b]->slines.size();
    for (uint64_t k = 0; k < kc[b];) {
      uint64_t take = std::min<uint64_t>(kc[b] - k, used < budget ? (budget - used) / bound[b] : 0);
      take = std::min<uint64_t>(take, (max_lines - lines) / nr);
      if (take == 0) {
        if (!win.empty()) {
          flush();
          continue;
        }
        take = 1; /* one record above the budget: a window of its own */
      }
      win.push_back(wga_maf_chunk_block{t.row0[b], k, k + take, nr, 0});
      used += take * bound[b];
      lines += take * nr;
      k += take;
    }
  }
  flush();
}

/* a piece with non-ASCII rows (the host reader took it: K14 marks them WGA_MAF_FALLBACK), on the host as the reference does it:
 * sizes count characters, a slice that splits a character panics (str slicing) */
static std::string chunk_host(const std::vector<MafRecord>& recs, uint64_t L, std::string& panic) {
  std::string t;
  auto boundary = [](const MafSLine& s, uint64_t i) {
    return i >= s.seq_size() || ((unsigned char)s.seq_data()[i] & 0xC0u) != 0x80u;
  };
  for (const MafRecord& r : recs) {
    const uint64_t bl = r.slines[0].seq_size(), nk = chunk_count(bl, L);
    std::vector<uint64_t> ends;
    for (const MafSLine& s : r.slines) ends.push_back(s.start);
    for (uint64_t k = 0; k < nk; k++) {
      const uint64_t c0 = k * L, c1 = bl - c0 > L ? c0 + L : bl;
      std::string rec = "a score=255\n";
      for (size_t i = 0; i < r.slines.size(); i++) {
        const MafSLine& s = r.slines[i];
        if (s.seq_size() < c1) {
          panic = kChunkShortRow;
          return t;
        }
        if (!boundary(s, c0) || !boundary(s, c1)) {
          panic = "panic: a chunk boundary falls inside a character (chunk.rs:75 byte index is not a char boundary)";
          return t;
        }
        uint64_t size = 0;
        for (uint64_t x = c0; x < c1; x++) {
          const unsigned char ch = (unsigned char)s.seq_data()[x];
          size += ch != '-' && (ch & 0xC0u) != 0x80u;
        }
        rec += "s\t" + s.name + "\t" + std::to_string(ends[i]) + "\t" + std::to_string(size) + (s.neg ? "\t-\t" : "\t+\t") +
               std::to_string(s.size) + "\t";
        rec.append(s.seq_data() + c0, (size_t)(c1 - c0));
        rec += "\n";
        ends[i] += size;
      }
      t += rec + "\n";
    }
  }
  return t;
}

int cmd_chunk(const std::string* input, uint64_t L, Output& out) {
  std::vector<uint64_t> kc; /* of the piece at hand */
  return maf_pieces(
      input, "#maf version=1.6 split_length=" + std::to_string(L), "WGA_MAF_CHUNK_OUT_BYTES", out, /* chunk.rs:29-30 */
      [&](const MafPiece& p, int, Dev& dg, bool in_place, uint32_t lo, uint32_t hi, const MafSink& sink) {
        chunk_blocks(dg, p.in, in_place, p.recs.data() + lo, hi - lo, kc.data() + lo, L, p.budget, sink);
        return false;
      },
      std::string(),
      [&](MafPiece& p, Output& o) {
        bool non_ascii = false;
        if (!p.in.on_device)
          for (const MafRecord* r : p.recs)
            for (const MafSLine& s : r->slines)
              for (size_t x = 0; x < s.seq_size() && !non_ascii; x++) non_ascii = (unsigned char)s.seq_data()[x] >= 0x80u;
        if (non_ascii) {
          o.write(chunk_host(p.in.recs, L, p.error));
          p.n = 0;
          return;
        }
        bool panic = false;
        p.n = chunk_plan(p.recs.data(), (uint32_t)p.recs.size(), L, kc, &panic);
        if (panic) p.error = kChunkShortRow;
      });
}
