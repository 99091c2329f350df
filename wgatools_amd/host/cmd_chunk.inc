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

/* the records of blocks recs[0 .. n) (kc[b] chunks each) on device d, window by window; sink(dev, text, bytes) takes every
 * window's text in order */
static void chunk_blocks(Dev& d, const MafInput& in, bool in_place, const MafRecord* const* recs, uint32_t n, const uint64_t* kc,
                         uint64_t L, size_t budget, const std::function<void(Dev&, const uint8_t*, size_t)>& sink) {
  d.init();
  std::vector<wga_maf_chunk_row> rows;
  std::vector<uint64_t> row0(n), bound(n);
  std::string blob;
  for (uint32_t b = 0; b < n; b++) {
    const MafRecord& r = *recs[b];
    row0[b] = rows.size();
    const uint64_t w = std::min<uint64_t>(L, r.slines[0].seq_size());
    uint64_t rb = 13;
    for (const MafSLine& s : r.slines) {
      wga_maf_chunk_row x;
      if (in_place) {
        x.seq_off = s.seq_off;
        x.name_off = s.name_off;
      } else { /* the rows gathered from the host copy of the text (the host reader, or a device other than the reader's) */
        x.name_off = blob.size();
        blob += s.name;
        x.seq_off = blob.size();
        blob.append(s.seq_data(), s.seq_size());
      }
      x.seq_len = s.seq_size();
      x.start = s.start;
      x.src_size = s.size;
      x.name_len = (uint32_t)s.name.size();
      x.strand_neg = s.neg ? 1u : 0u;
      rows.push_back(x);
      rb += s.name.size() + 70u + w;
    }
    bound[b] = rb;
  }
  const uint8_t* d_text = in_place ? in.d_text : nullptr;
  if (!in_place) {
    blob.append(16, '\0');
    d_text = d.upload((const uint8_t*)blob.data(), blob.size());
  }
  auto* d_rows = d.upload(rows);
  auto* d_carry = (uint64_t*)d.alloc(std::max<size_t>(rows.size(), 1) * 8);
  d.check(wga_memset(d.ctx, d_carry, 0, std::max<size_t>(rows.size(), 1) * 8));
  g_timer.mark("host rows + upload");
  std::vector<wga_maf_chunk_block> win;
  uint64_t used = 0, lines = 0;
  auto flush = [&]() {
    if (win.empty()) return;
    auto* d_blocks = d.upload(win);
    void* d_work = d.alloc((size_t)wga_maf_chunk_work_bytes((uint32_t)win.size(), lines));
    uint64_t bytes = 0;
    d.check(wga_maf_chunk(d.ctx, d_text, d_rows, (uint32_t)win.size(), d_blocks, lines, L, d_carry, d_work, &bytes, nullptr));
    auto* d_out = (uint8_t*)d.alloc((size_t)bytes + 16);
    d.check(wga_maf_chunk(d.ctx, d_text, d_rows, (uint32_t)win.size(), d_blocks, lines, L, d_carry, d_work, &bytes, d_out));
    d.release(d_work);
    d.release(d_blocks);
    sink(d, d_out, (size_t)bytes); /* the sink releases d_out or keeps it */
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
      win.push_back(wga_maf_chunk_block{row0[b], k, k + take, nr, 0});
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
  Dev d;
  MafDevices md(d); /* --gpus N: a piece's blocks in contiguous ranges over the devices, the text written in block order */
  size_t budget = (size_t)1 << 28;
  if (const char* e = getenv("WGA_MAF_CHUNK_OUT_BYTES")) budget = std::max<size_t>(1, (size_t)strtoull(e, nullptr, 10));
  std::string pending_error;
  MafChunks chunks(input);
  chunks.keep_going = true;
  out.write("#maf version=1.6 split_length=" + std::to_string(L) + "\n"); /* chunk.rs:29-30: the input's header is dropped */
  MafInput min;
  g_timer.mark("host");
  for (;;) {
    bool more = false;
    try {
      more = chunks.next(d, min);
    } catch (Error& e) {
      pending_error = e.msg;
    }
    g_timer.mark("read + upload + split");
    if (!more) break;
    const std::vector<const MafRecord*> all = all_records(min.recs);
    bool non_ascii = false;
    if (!min.on_device)
      for (const MafRecord* r : all)
        for (const MafSLine& s : r->slines)
          for (size_t x = 0; x < s.seq_size() && !non_ascii; x++) non_ascii = (unsigned char)s.seq_data()[x] >= 0x80u;
    if (non_ascii) {
      std::string panic;
      out.write(chunk_host(min.recs, L, panic));
      if (!panic.empty()) pending_error = panic;
    } else {
      std::vector<uint64_t> kc;
      bool panic = false;
      const uint32_t n = chunk_plan(all.data(), (uint32_t)all.size(), L, kc, &panic);
      const int ng = md.count();
      if (ng == 1) {
        chunk_blocks(d, min, min.on_device, all.data(), n, kc.data(), L, budget, [&](Dev& dg, const uint8_t* t, size_t bytes) {
          stream_out(dg, out, t, bytes);
          dg.release((void*)t);
        });
      } else {
        /* device 0's windows are the first text of the piece: they leave as they are made (its worker thread is the only one
         * writing while the devices work); the other devices keep their windows in HBM until the devices in front of them are done */
        std::vector<std::vector<std::pair<const uint8_t*, size_t>>> texts(ng);
        on_devices(ng, [&](int g) {
          const uint32_t lo = (uint32_t)((uint64_t)n * g / ng), hi = (uint32_t)((uint64_t)n * (g + 1) / ng);
          if (lo == hi) return;
          chunk_blocks(md.dev(g), min, g == 0 && min.on_device, all.data() + lo, hi - lo, kc.data() + lo, L, budget,
                       [&](Dev& dg, const uint8_t* t, size_t bytes) {
                         if (g == 0) {
                           stream_out(dg, out, t, bytes, false);
                           dg.release((void*)t);
                         } else {
                           texts[g].emplace_back(t, bytes);
                         }
                       });
        });
        for (int g = 0; g < ng; g++)
          for (const auto& t : texts[g]) stream_out(md.dev(g), out, t.first, t.second);
      }
      if (panic) pending_error = kChunkShortRow;
    }
    md.release_all();
    if (pending_error.empty() && !min.error.empty()) pending_error = min.error;
    if (!pending_error.empty()) break;
  }
  out.close();
  g_timer.mark("write");
  if (!pending_error.empty()) fail(pending_error);
  return leave(0);
}
