/*
 * wga_capi.cpp — the C-ABI of libwgahip.so (include/wga_hip.h): the context, what every launcher shares (the grow-only device
 * buffer, the scan driver, the count -> fill cache) and the entry points for context, stream, parameters, memory and copies.
 * The launch logic of the kernels is in the capi_*.inc parts, one per kernel family, included at the end: one translation
 * unit.  Compiled as HIP for gfx950 (product) or, with -DWGA_EMU, as plain C++ over tests/emu/simt_emu.h (CPU logic tests only).
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <utility>
#include <vector>

/* the kernels, one header per family (each names the reference code it replaces), in dependency order: a header may use helpers
 * of the ones in front of it */
#include <type_traits>

#include "wga_kernels.h"       /* the core: types, wave and block scans, the row pre-pass, the paf2maf layout */
#include "wga_k1_stat.h"       /* K1: the stat walk */
#include "wga_scan.h"          /* the generic scan of every count -> fill launcher (run_scan) */
#include "wga_k2_v1.h"         /* v1 of the row kernel: expand_variant 0 and the tiles K2s leaves */
#include "wga_kernels_k2s.h"   /* K2s: the streaming row kernel (paf2maf, pafpseudo's rows) */
#include "wga_k_class.h"
#include "wga_k_peers.h"       /* the multi-GPU counter reduction */
#include "wga_k5_pafcov.h"
#include "wga_k6_pafpseudo.h"
#include "wga_k3_maf.h"        /* K3 / K4: the MAF walks */
#include "wga_k7_paf_call.h"
#include "wga_k8_tokenise.h"
#include "wga_text_out.h"      /* what the text writers share: decimals, sinks, the staged stretch */
#include "wga_chain_items.h"   /* the items of a stream of chains (K25, K27, K28), a data line's CIGAR text (K11, K27) */
#include "wga_paf_head.h"      /* a PAF record's columns and csv quoting (K27, K28) */
#include "wga_k9_bed.h"
#include "wga_k10_chain.h"
#include "wga_k11_bridges.h"
#include "wga_k12_dotplot.h"
#include "wga_k13_splitters.h"
#include "wga_k15_fasta.h"
#include "wga_k18_bgzf_deflate.h"
#include "wga_k16_paf_call_vcf.h" /* K16: the VCF rows of call on PAF */
#include "wga_k17_bgzf_inflate.h" /* K17: BGZF inflate */
#include "wga_k19_maf_call.h"  /* K19: rules and VCF rows of call on MAF */
#include "wga_k20_maf_chunk.h" /* K20: chunk on MAF */
#include "wga_k21_maf_slice.h" /* K21: maf-ext's slices */
#include "wga_k22_maf_rewrite.h" /* K22: filter and rename on MAF */
#include "wga_k23_chain_split.h" /* K23: the chain line splitter */
#include "wga_k24_paf_filter.h" /* K24: filter on PAF, the pair sums of `-a` */
#include "wga_k25_chain_write.h" /* K25: the chain record writer of filter on chain */
#include "wga_k26_dotplot_csv.h" /* K26: the base-level csv rows of dotplot */
#include "wga_k27_chain2paf.h" /* K27: the PAF record writer of chain2paf */
#include "wga_k28_maf2paf.h" /* K28: the PAF record writer of maf2paf */
#include "wga_k29_paf_fix.h" /* K29: the end-fixing line writer of validate --fix */
#include "wga_k30_chain_heads.h" /* K30: the chain heads of paf2chain and maf2chain */
#include "wga_k31_pseudo_frame.h" /* K31: the row frame writer of pafpseudo */
#include "wga_k32_maf_frame.h" /* K32: the MAF record frames of paf2maf and chain2maf */
#include "wga_k33_stat_rows.h" /* K33: the TSV rows of stat --each, the f32 text */
#include "wga_k34_dotplot_overview.h" /* K34: the csv rows of dotplot -m overview, the f64 text */
#include "wga_sort.h"          /* the stable key sort (run_sort_u32) */
#include "wga_k35_maf_index.h" /* K35: maf-index: block offsets, name groups, the JSON interval text */
#include "wga_group.h"         /* group-by on the device (run_group) */
#include "wga_k36_stat_pairs.h" /* K36: stat's merged table: pair groups, sums, the pairs' rows */

/* A grow-only device buffer of a context.  reserve() leaves it with room for `need` bytes: one that is too small is freed
 * behind the work of the context's stream and allocated anew with `grow` (>= need) bytes — every site has its own growth rule —,
 * its contents are gone and *grew says so. */
struct DevBuf {
  void* mem = nullptr;
  size_t cap = 0; /* bytes */
  int reserve(wga_ctx* c, size_t need, size_t grow, bool* grew = nullptr);
  void release() {
    if (mem) (void)rt_free(mem);
    mem = nullptr, cap = 0;
  } /* by wga_ctx_destroy, not by a destructor: a launch of the emulator build copies the structs whose fields it names */
};

/* What a count call of the two-call protocol leaves on the context for its fill call is kept under a key: who built it, the
 * device arrays it was built from (with their extent in bytes where the caller knows it: the packed ops, the CSR offsets; 0 =
 * one byte at the start, for the per-record arrays of an entry point's own layout) and the parameters. */
struct CallKey {
  int who = 0; /* the kernel or entry point of the cache's family that built it */
  struct Arr {
    const void* p = nullptr;
    size_t bytes = 0;
  } arr[5];
  uint64_t par[6] = {0, 0, 0, 0, 0, 0};
  bool operator==(const CallKey& o) const {
    bool same = who == o.who;
    for (int k = 0; k < 5; k++) same = same && arr[k].p == o.arr[k].p && arr[k].bytes == o.arr[k].bytes;
    for (int k = 0; k < 6; k++) same = same && par[k] == o.par[k];
    return same;
  }
};
struct CallCache {
  CallKey key;
  bool valid = false;
  /* a fill call under the same key takes what is kept; whatever the answer, nothing is kept any longer (one shot: a hit consumes
   * it, a miss rebuilds it) until keep() */
  bool take(const CallKey& k, bool is_fill) {
    const bool hit = is_fill && valid && key == k;
    valid = false;
    return hit;
  }
  void keep(const CallKey& k) { key = k, valid = true; }
  /* [lo, lo + bytes) is written or freed (bytes == 0: the allocation that starts at lo): a keyed array that overlaps it — a write
   * anywhere inside a known extent, a write that covers the start of the others — drops what is kept */
  void written(const void* lo, size_t bytes) {
    const uintptr_t a = (uintptr_t)lo, z = a + (bytes ? bytes : 1);
    for (const CallKey::Arr& q : key.arr)
      if (q.p && (uintptr_t)q.p < z && (uintptr_t)q.p + (q.bytes ? q.bytes : 1) > a) valid = false;
  }
};

struct wga_ctx {
  int device = 0;
  wga_stream_t own_stream = nullptr;
  wga_stream_t stream = nullptr;
  int expand_force_slow = 0;
  int expand_no_table = 0;
  unsigned expand_drain_min = 0; /* v1 only: 0 = by the size of the pools (WGA_DRAIN_POOL_BYTES: 32, 16 for genome-sized pools) */
  unsigned expand_drain_min_used = 0;
  uint64_t op_long_ops = 16384;  /* op walks with one wave per record (K7 call events, K12 dotplot segments): records beyond this many ops ... */
  uint64_t op_piece_ops = 8192;  /* ... are walked in pieces of this many (a multiple of 256), one wave each (test knobs: "op_long_ops", "op_piece_ops") */
  uint64_t maf_long_cols = 32768;  /* MAF blocks beyond this many columns are walked piece by piece ... */
  uint64_t maf_piece_cols = 16384; /* ... of this many columns, one wave each (test knobs: "maf_long_cols", "maf_piece_cols") */
  unsigned paf_pair_hash_bits = 64; /* K24: the low bits of the pair hash that pick a slot (test knob "paf_pair_hash_bits": few bits make the pairs collide) */
  unsigned maf_index_hash_bits = 64; /* K35: the low bits of the name hash that pick a slot (test knob "maf_index_hash_bits") */
  unsigned maf_index_sort_bits = 8;  /* K35: the digit width of the sort by group (test knob "maf_index_sort_bits": any width gives the same order) */
  unsigned stat_pair_hash_bits = 64; /* K36: the low bits of the pair hash that pick a slot (test knob "stat_pair_hash_bits") */
  unsigned maf_group = 0;          /* blocks per wave of the MAF stream kernels, 1 .. 8 ("maf_group"; 0 = by the number of blocks) */
  DevBuf maf_tab;                  /* K3 / K4: the table of a call's long blocks (header, list, pieces) */
  bool maf_hdr_clean = false;      /* the header's append counters are zero (the plan kernel leaves them so) */
  CallCache maf_cache;             /* the table of a count call, for the fill call on the same arrays */
  int expand_variant = -1; /* the row kernel: -1 / 3 the streaming kernel (wga_kernels_k2s.h), 0 v1 (wga_k2_v1.h: what the
                              streaming kernel leaves is v1's in either case).  The window kernel of rounds 3-5 (2) is gone: it was
                              ahead only below 100 ops per record (30-op records 6.1 against 7.3 ms) */
  int expand_variant_used = 0;
  int expand_job_tiles = 0; /* streaming kernel: tiles per wave ("expand_job_tiles"); 0 = by the batch (job_tiles_for) */
  int pseudo_variant = 3;   /* pafpseudo's rows: 3 the streaming row kernel, 0 one block per tile ("pseudo_variant") */
  const u32* pseudo_counts = nullptr; /* ... the two counters of the tiles its last launch left to the block kernel */
  const u32* stream_counts = nullptr; /* streaming kernel: the two counters of the tiles its last launch left to v1 (in the scratch arena) */
  DevBuf scratch;
  /* the piece table of the op walks over long records (K7, K10, K12): built by the count call of the two-call protocol and
   * kept for the fill call on the same batch with the same parameters (the key), in a buffer of its own */
  struct OpTab {
    DevBuf buf;
    CallCache cache;
    uint32_t np = 0;
    bool all = false;         /* every record is in the table (the one-wave kernel is not launched) */
    u64* piece_off = nullptr; /* n + 1 */
    u32* piece_rec = nullptr; /* np: the record of every piece */
    void* pieces = nullptr;   /* np x per_piece bytes */
  } op_tab;
  struct ClassTab { /* pafpseudo: the tile and record class sums of wga_cigar_class_sums, kept for wga_pafpseudo_fill */
    DevBuf buf;
    CallCache cache;
    wga_tile_sum* tiles = nullptr;
    wga_class_sums* rec_sums = nullptr;
  } class_tab;
  struct ElemScan { /* K11: the count call's scan of the element sizes, kept for the fill call */
    DevBuf buf;
    CallCache cache;
  } elem_scan;
  struct Cov { /* pafcov */
    DevBuf pieces;    /* the pieces' descriptors (wga_cov_desc) in window order */
    DevBuf tile_list; /* WGA_COV_TILE_CAP piece slots per tile of ops */
    DevBuf order;     /* the order the marks -> counts replay takes the windows in, kept for the ranges it was made for */
    std::vector<u64> order_key;
    DevBuf list;      /* the pieces beyond a tile's slots (WGA_COV_LISTS regions of list_rcap) */
    u64 list_rcap = 0;
  } cov;
  /* wga_reduce_scatter_i32: events that order this context's stream against the other devices' (created at first use), a
   * stream per staged pull, and what the two test switches say */
  bool rs_have_ev = false;
  rt_event_t rs_ready, rs_done;
  std::vector<wga_stream_t> rs_streams;
  std::vector<rt_event_t> rs_copied;
  bool rs_same_device_ok = false; /* "reduce_same_device_ok": distinct contexts may share a device (one-GPU test boxes) */
  bool rs_staged = false;         /* "reduce_staged": pull into scratch over N-1 streams instead of reading the peers in place */
#ifdef WGA_EMU
  u32 cov_spin_limit = 64; /* the emulator runs one block at a time: a tile that is not there yet will not come while this one polls */
#else
  u32 cov_spin_limit = 1u << 12;
#endif /* polls of a tile sum (milliseconds of waiting where ten microseconds are the rule) before the
                                    look-back adds up the ops itself (parameter "cov_spin_limit") */
  /* optional per-launch timing of the expand kernel proper (events on the launch stream) */
  static const int kTimingRing = 64;
  bool timing = false;
  rt_event_t ev[2 * kTimingRing];
  uint32_t ev_n = 0;
};

static thread_local std::string g_last_error;

static int fail(int code, const char* what, const char* detail) {
  g_last_error = std::string(what) + (detail ? std::string(": ") + detail : std::string());
  return code;
}
#define RT_CHECK(expr)                                      \
  do {                                                      \
    const char* _e = (expr);                                \
    if (_e) return fail(WGA_E_HIP, #expr, _e);              \
  } while (0)
#define LAUNCH_CHECK()                                      \
  do {                                                      \
    const char* _e = rt_launch_error();                     \
    if (_e) return fail(WGA_E_HIP, "kernel launch", _e);    \
  } while (0)

static int ctx_bind(wga_ctx* c) {
  if (!c) return fail(WGA_E_INVALID_ARG, "null context", nullptr);
  RT_CHECK(rt_set_device(c->device));
  return WGA_OK;
}

int DevBuf::reserve(wga_ctx* c, size_t need, size_t grow, bool* grew) {
  if (grew) *grew = cap < need;
  if (cap >= need) return WGA_OK;
  RT_CHECK(rt_sync(c->stream)); /* work in flight may still use the old one */
  if (mem) RT_CHECK(rt_free(mem));
  mem = nullptr, cap = 0;
  RT_CHECK(rt_malloc(&mem, grow));
  cap = grow;
  return WGA_OK;
}

/* grow-only scratch arena on the context (scan partials etc.) */
static int ctx_scratch(wga_ctx* c, size_t bytes, void** out) {
  /* whoever takes the scratch may overwrite the two counters the last row-kernel launch left in it: "expand_stream_left_to_v1"
   * and "pseudo_stream_left_to_blocks" then answer "not known" instead of reading someone else's bytes (the launches that own
   * the counters set the pointers again behind this call) */
  c->stream_counts = nullptr;
  c->pseudo_counts = nullptr;
  int rc = c->scratch.reserve(c, bytes, bytes < (1u << 20) ? (1u << 20) : bytes + bytes / 2);
  *out = c->scratch.mem;
  return rc;
}

/* the exclusive scan of f(0 .. n - 1) into d_out[0 .. n] (the total last): the one place that launches the scan kernels */
template <typename F>
static int run_scan_ws(wga_ctx* c, F f, u32 n, u64* d_out /* n+1 */, u64* partial /* n/1024 + 2 */) {
  u32 nb = (u32)(((u64)n + 1023u) / 1024u); /* n may lie within 1023 of 2^32 */
  if (nb) {
    WGA_LAUNCH(k_scan_partials<F>, nb, WGA_BLOCK, c->stream, f, n, partial);
    LAUNCH_CHECK();
  }
  WGA_LAUNCH(k_scan_top, 1, WGA_BLOCK, c->stream, partial, nb, d_out + n);
  LAUNCH_CHECK();
  if (nb) {
    WGA_LAUNCH(k_scan_final<F>, nb, WGA_BLOCK, c->stream, f, n, (const u64*)partial, d_out);
    LAUNCH_CHECK();
  }
  return WGA_OK;
}
/* ... with its partials in the context scratch */
template <typename F>
static int run_scan(wga_ctx* c, F f, u32 n, u64* d_out /* n+1 */) {
  void* ws;
  int rc = ctx_scratch(c, ((size_t)(n + 1023u) / 1024u + 1) * sizeof(u64), &ws);
  if (rc) return rc;
  return run_scan_ws(c, f, n, d_out, (u64*)ws);
}
/* The stable sort of the n payloads in buf[0] by key(payload), a key of key_bits bits, in passes of digit_bits bits (wga_sort.h):
 * *where = the one of buf[0] / buf[1] that holds the result (buf[0] when there is nothing to sort by).  cnt: sort_cnt_words(n) words
 * for the digit counts and their scan, partial: that scan's partials (sort_cnt_words(n) / 1024 + 2 words). */
static size_t sort_blocks(uint64_t n) { return (size_t)((n + WGA_SORT_ITEMS - 1u) / WGA_SORT_ITEMS); }
static size_t sort_cnt_words(uint64_t n) { return ((size_t)1 << WGA_SORT_MAX_BITS) * sort_blocks(n) + 1; }
template <typename K>
static int run_sort_u32(wga_ctx* c, K key, u32 n, unsigned key_bits, unsigned digit_bits, u32* const buf[2], u64* cnt, u64* partial,
                        int* where) {
  *where = 0;
  if (n == 0) return WGA_OK;
  const u32 nblk = (u32)sort_blocks(n);
  for (unsigned shift = 0; shift < key_bits; shift += digit_bits) {
    const u32 bits = std::min(digit_bits, key_bits - shift);
    const u32* in = buf[*where];
    u32* out = buf[*where ^ 1];
    WGA_LAUNCH(k_sort_hist<K>, nblk, WGA_BLOCK, c->stream, key, in, n, (u32)shift, bits, nblk, cnt);
    LAUNCH_CHECK();
    ScanPlain f;
    f.in = cnt;
    int rc = run_scan_ws(c, f, (u32)(((size_t)1 << bits) * nblk), cnt, partial); /* in place, as delim_lists does */
    if (rc) return rc;
    WGA_LAUNCH(k_sort_scatter<K>, nblk, WGA_BLOCK, c->stream, key, in, n, (u32)shift, bits, nblk, (const u64*)cnt, out);
    LAUNCH_CHECK();
    *where ^= 1;
  }
  return WGA_OK;
}
/* The groups of n items by key (wga_group.h): rounds of claim and settle until every item has its group's lowest member in rep[],
 * then the scan that numbers the groups.  It leaves *n_groups (a host value: the call synchronises), every item's group number in
 * `start` (the start slots are done with) and the items 0 .. n - 1 in list[0], ready for run_sort_u32.  slots: group_slots(n) words;
 * rep, start, list[0], list[1]: n each; gidx: n + 1; partial: the scan's (n / 1024 + 2 words). */
template <typename K>
static int run_group(wga_ctx* c, K key, u32 n, unsigned hash_bits, GroupHdr* hdr, u64* slots, u32* rep, u32* start, u32* const list[2],
                     u64* gidx, u64* partial, u64* n_groups) {
  *n_groups = 0;
  if (n == 0) return WGA_OK;
  const u64 M = group_slots(n);
  const u32 slot_mask = (u32)(M - 1u);
  const u64 hash_mask = hash_bits >= 64u ? ~0ull : (1ull << hash_bits) - 1ull;
  const u32 grid = (u32)(((u64)n + 255u) / 256u);
  RT_CHECK(rt_memset(slots, 0xFF, (size_t)M * sizeof(u64), c->stream));
  WGA_LAUNCH(k_group_init<K>, grid, WGA_BLOCK, c->stream, key, (u64)n, hash_mask, slot_mask, start, rep, list[0]);
  LAUNCH_CHECK();
  u64 m = n;
  for (u64 r = 0; m; r++) { /* every round gives the lowest item of each start slot's class a group, or steps over a taken slot */
    if (m > n || r > 2u * M + 64u) return fail(WGA_E_HIP, "the group table did not settle", nullptr);
    const u32 g = (u32)((m + 255u) / 256u);
    WGA_LAUNCH(k_group_claim, g, WGA_BLOCK, c->stream, (const u32*)list[r & 1u], m, r, slot_mask, (const u32*)start, slots, hdr);
    LAUNCH_CHECK();
    WGA_LAUNCH(k_group_settle<K>, g, WGA_BLOCK, c->stream, key, (const u32*)list[r & 1u], m, (u64)n, r, slot_mask, (const u32*)start,
               (const u64*)slots, rep, list[(r + 1u) & 1u], hdr);
    LAUNCH_CHECK();
    RT_CHECK(rt_d2h(&m, &hdr->cnt[(r + 1u) & 1u], sizeof m, c->stream));
  }
  ScanGroupRep fr;
  fr.rep = rep;
  int rc = run_scan_ws(c, fr, n, gidx, partial);
  if (rc) return rc;
  u64 ng = 0;
  RT_CHECK(rt_d2h(&ng, gidx + n, sizeof ng, c->stream));
  if (ng == 0 || ng > n) return fail(WGA_E_HIP, "the groups' scan is not a scan", nullptr);
  WGA_LAUNCH(k_group_number, grid, WGA_BLOCK, c->stream, (u64)n, (const u32*)rep, (const u64*)gidx, start, list[0]);
  LAUNCH_CHECK();
  *n_groups = ng;
  return WGA_OK;
}
/* the text of a stream of n items of format f behind isc, the scan of their sizes over ScanItems<F> (wga_text_out.h) */
template <typename F>
static int run_text_items_fill(wga_ctx* c, const F& f, u32 n, const u64* isc, u64 total, uint8_t* d_out) {
  WGA_LAUNCH(k_text_items_fill<F>, (u32)(((u64)n + WGA_TEXT_ITEMS - 1u) / WGA_TEXT_ITEMS), WGA_BLOCK, c->stream, f, (u64)n, isc, total,
             d_out);
  LAUNCH_CHECK();
  return WGA_OK;
}
/* Both calls of a text of one row per record (RECORD ROWS in wga_text_out.h: K33, K34) behind the entry's own argument checks;
 * the row source's fields of f are the entry's.  d_work in u64 words, n rows: the plan (a row's bytes) [n] | the scan's partials
 * [n / 1024 + 4].  The count call (d_out null) plans, scans into d_row_off[n + 1] and reads the total back; the fill call writes
 * the text. */
static size_t record_rows_work_words(uint64_t n) { return (size_t)n + (size_t)(n / 1024u) + 4; }
template <typename F>
static int run_record_rows(wga_ctx* c, F f, u32 n, void* d_work, uint64_t* d_row_off, uint64_t* total_bytes, uint8_t* d_out) {
  if (!d_out) *total_bytes = 0;
  if (n == 0 || (d_out && *total_bytes == 0)) return WGA_OK;
  u64* plan = (u64*)d_work;
  f.plan = plan;
  f.n_rec = n;
  if (d_out) return run_text_items_fill(c, f, n, (const u64*)d_row_off, (u64)*total_bytes, d_out);
  WGA_LAUNCH(k_record_rows_plan<typename F::Src>, (u32)(((u64)n + 255u) / 256u), WGA_BLOCK, c->stream, f.names, f.n_name_bytes, f.heads, n, f.counts, plan);
  LAUNCH_CHECK();
  int rc = run_scan_ws(c, ScanItems<F>{f}, n, (u64*)d_row_off, plan + n);
  if (rc) return rc;
  u64 tot = 0;
  RT_CHECK(rt_d2h(&tot, d_row_off + n, sizeof tot, c->stream));
  *total_bytes = tot;
  return WGA_OK;
}
/* A formatter alone (k_bits_text: K33's f32, K34's f64) */
template <typename B, u32 kSlot, void (*kEmit)(TextPut&, B)>
static int run_bits_text(wga_ctx* c, uint64_t n, const B* d_bits, uint8_t* d_text, uint8_t* d_len) {
  int rc = ctx_bind(c);
  if (rc) return rc;
  if (n == 0) return WGA_OK;
  if (!d_bits || !d_text || !d_len) return fail(WGA_E_INVALID_ARG, "null array", nullptr);
  if (n > 0xFFFFFFF0ull) return fail(WGA_E_INVALID_ARG, "too many values", nullptr);
  WGA_LAUNCH((k_bits_text<B, kSlot, kEmit>), (u32)((n + 255u) / 256u), WGA_BLOCK, c->stream, (u64)n, d_bits, d_text, d_len);
  LAUNCH_CHECK();
  return WGA_OK;
}
/* What wga_chain_filter and wga_chain2paf do alike behind their own null checks: the checks of the arrays and limits, the count
 * call's zeroed results (n_kept: K25's, else null), the read of the data lines' number and the items of the stream (the plan leads
 * d_work in both layouts).  *n_items == 0 when it returns WGA_OK: nothing is left to do. */
static int chain_items_open(wga_ctx* c, const uint8_t* d_text, uint64_t n_bytes, const wga_chain_head* d_heads, uint64_t n_chains,
                            const uint64_t* d_lines, const uint64_t* d_line_off, void* d_work, const uint8_t* d_out,
                            uint64_t* total_bytes, uint64_t* n_kept, ChainItemBase* it, u32* n_items) {
  static_assert(sizeof(wga_chain_head) == sizeof(wga_chain_head_dev), "wga_chain_head layout");
  *n_items = 0;
  if (!d_work) return fail(WGA_E_INVALID_ARG, "d_work null", nullptr);
  if (n_chains > 0xFFFFFFF0ull || n_bytes >= 0xFFFFFFF0ull) return fail(WGA_E_INVALID_ARG, "a text within wga_chain_split's limits", nullptr);
  if (n_chains && (!d_text || !d_heads || !d_line_off)) return fail(WGA_E_INVALID_ARG, "null array", nullptr);
  if (!d_out) {
    *total_bytes = 0;
    if (n_kept) *n_kept = 0;
  }
  if (n_chains == 0 || (d_out && *total_bytes == 0)) return WGA_OK;
  u64 nd = 0; /* the data lines: the last offset */
  RT_CHECK(rt_d2h(&nd, d_line_off + n_chains, sizeof nd, c->stream));
  if (nd > 0xFFFFFFF0ull || n_chains + nd > 0xFFFFFFF0ull) return fail(WGA_E_INVALID_ARG, "more than 0xFFFFFFF0 chains and data lines", nullptr);
  if (nd && !d_lines) return fail(WGA_E_INVALID_ARG, "d_lines null", nullptr);
  it->lines = (const u64*)d_lines;
  it->line_off = (const u64*)d_line_off;
  it->plan = (const u64*)d_work;
  it->n_rec = (u32)n_chains;
  it->n_lines = nd;
  *n_items = (u32)(n_chains + nd);
  return WGA_OK;
}

static int check_batch(const wga_cigar_batch* b) {
  if (!b) return fail(WGA_E_INVALID_ARG, "batch is null", nullptr);
  if (b->n && (!b->d_op_off || !b->d_strand_neg)) return fail(WGA_E_INVALID_ARG, "batch arrays null", nullptr);
  if (b->n_ops && !b->d_ops) return fail(WGA_E_INVALID_ARG, "d_ops null", nullptr);
  if (((uintptr_t)b->d_ops & 15u) != 0) return fail(WGA_E_INVALID_ARG, "d_ops must be 16-byte aligned", nullptr);
  return WGA_OK;
}
static inline u64 n_tiles(u64 n_ops) { return (n_ops + WGA_TILE - 1) / WGA_TILE; }

extern "C" {

int wga_abi_version(void) { return WGA_ABI_VERSION; }
const char* wga_last_error(void) { return g_last_error.c_str(); }
int wga_device_count(void) { return rt_device_count(); }

int wga_ctx_create(int device, wga_ctx** out) {
  if (!out) return fail(WGA_E_INVALID_ARG, "out is null", nullptr);
  int n = rt_device_count();
  if (n <= 0) return fail(WGA_E_NO_DEVICE, "no HIP device visible (libwgahip needs an MI355X)", nullptr);
  if (device < 0 || device >= n) return fail(WGA_E_INVALID_ARG, "device index out of range", nullptr);
  wga_ctx* c = new wga_ctx();
  c->device = device;
  const char* e = rt_set_device(device);
  if (!e) e = rt_stream_create(&c->own_stream);
  if (e) {
    delete c;
    return fail(WGA_E_HIP, "context creation", e);
  }
  c->stream = c->own_stream;
  /* A/B switch for measurements: WGA_EXPAND_VARIANT=0 selects v1 of the paf2maf row kernel (wga_ctx_set_param overrides) */
  if (const char* v = getenv("WGA_EXPAND_VARIANT")) c->expand_variant = (atoi(v) == 0 || atoi(v) == 3) ? atoi(v) : -1;
  if (const char* v = getenv("WGA_EXPAND_DRAIN_MIN")) {
    const int d = atoi(v);
    if (d >= 0 && d <= 64) c->expand_drain_min = (unsigned)d;
  }
  *out = c;
  return WGA_OK;
}

void wga_ctx_destroy(wga_ctx* c) {
  if (!c) return;
  (void)rt_set_device(c->device);
  (void)rt_sync(c->stream);
  if (c->timing)
    for (int k = 0; k < 2 * wga_ctx::kTimingRing; k++) rt_event_destroy(c->ev[k]);
  if (c->rs_have_ev) rt_event_destroy(c->rs_ready), rt_event_destroy(c->rs_done);
  for (rt_event_t e : c->rs_copied) rt_event_destroy(e);
  for (wga_stream_t st : c->rs_streams) rt_stream_destroy(st);
  for (DevBuf* b : {&c->scratch, &c->maf_tab, &c->op_tab.buf, &c->class_tab.buf, &c->elem_scan.buf, &c->cov.pieces,
                    &c->cov.tile_list, &c->cov.order, &c->cov.list})
    b->release();
  rt_stream_destroy(c->own_stream);
  delete c;
}

/* The context's scratch arenas are ordered on ONE stream: work still in flight on the stream that is being left must
 * not see them reused or regrown by calls on the new one, so a switch drains the old stream first. */
int wga_ctx_set_stream(wga_ctx* c, void* hip_stream) {
  int rc = ctx_bind(c);
  if (rc) return rc;
#ifdef WGA_EMU
  (void)hip_stream; /* a caller's stream handle means nothing to the emulator: everything runs in call order anyway */
  return WGA_OK;
#else
  if (c->stream != (wga_stream_t)hip_stream) RT_CHECK(rt_sync(c->stream));
  c->stream = (wga_stream_t)hip_stream;
  return WGA_OK;
#endif
}

int wga_ctx_reset_stream(wga_ctx* c) {
  int rc = ctx_bind(c);
  if (rc) return rc;
  if (c->stream != c->own_stream) RT_CHECK(rt_sync(c->stream));
  c->stream = c->own_stream;
  return WGA_OK;
}

int wga_ctx_set_param(wga_ctx* c, const char* name, int64_t value) {
  if (!c || !name) return fail(WGA_E_INVALID_ARG, "null argument", nullptr);
  if (strcmp(name, "expand_force_slow") == 0) {
    c->expand_force_slow = value != 0;
    return WGA_OK;
  }
  if (strcmp(name, "reduce_same_device_ok") == 0) { /* wga_reduce_scatter_i32 over contexts that share a device (tests) */
    c->rs_same_device_ok = value != 0;
    return WGA_OK;
  }
  if (strcmp(name, "cov_spin_limit") == 0) { /* K5's list pass: polls of a tile sum before the look-back adds up the ops itself */
    if (value < 0 || value > 0x7FFFFFFF) return fail(WGA_E_INVALID_ARG, "cov_spin_limit: 0 .. 2^31 - 1", nullptr);
    c->cov_spin_limit = (u32)value;
    return WGA_OK;
  }
  if (strcmp(name, "reduce_staged") == 0) { /* wga_reduce_scatter_i32 by staged peer copies even where peer access exists */
    c->rs_staged = value != 0;
    return WGA_OK;
  }
  if (strcmp(name, "expand_drain_min") == 0) { /* 0 = chosen by the size of the sequence pools (WGA_DRAIN_POOL_BYTES) */
    if (value < 0 || value > 64) return fail(WGA_E_INVALID_ARG, "expand_drain_min: 0 .. 64", nullptr);
    c->expand_drain_min = (unsigned)value;
    return WGA_OK;
  }
  if (strcmp(name, "expand_no_table") == 0) {
    c->expand_no_table = value != 0;
    return WGA_OK;
  }
  if (strcmp(name, "op_long_ops") == 0) {
    if (value < 1) return fail(WGA_E_INVALID_ARG, "must be positive", name);
    c->op_long_ops = (uint64_t)value;
    return WGA_OK;
  }
  if (strcmp(name, "op_piece_ops") == 0) {
    if (value < 256 || (value & 255)) return fail(WGA_E_INVALID_ARG, "a positive multiple of 256", name);
    c->op_piece_ops = (uint64_t)value;
    return WGA_OK;
  }
  if (strcmp(name, "maf_long_cols") == 0 || strcmp(name, "maf_piece_cols") == 0) {
    if (value < 1) return fail(WGA_E_INVALID_ARG, "must be positive", name);
    (name[4] == 'l' ? c->maf_long_cols : c->maf_piece_cols) = (uint64_t)value;
    return WGA_OK;
  }
  if (strcmp(name, "maf_group") == 0) {
    if (value < 0 || value > (long long)WGA_MAF_G) return fail(WGA_E_INVALID_ARG, "maf_group: 0 (by the batch) .. 8", nullptr);
    c->maf_group = (unsigned)value;
    return WGA_OK;
  }
  if (strcmp(name, "paf_pair_hash_bits") == 0) { /* wga_paf_pairs: the hash is cut to this many low bits before it picks a place */
    if (value < 1 || value > 64) return fail(WGA_E_INVALID_ARG, "paf_pair_hash_bits: 1 .. 64", nullptr);
    c->paf_pair_hash_bits = (unsigned)value;
    return WGA_OK;
  }
  if (strcmp(name, "maf_index_hash_bits") == 0) { /* wga_maf_index: the hash is cut to this many low bits before it picks a place */
    if (value < 1 || value > 64) return fail(WGA_E_INVALID_ARG, "maf_index_hash_bits: 1 .. 64", nullptr);
    c->maf_index_hash_bits = (unsigned)value;
    return WGA_OK;
  }
  if (strcmp(name, "stat_pair_hash_bits") == 0) { /* wga_stat_pairs: the hash is cut to this many low bits before it picks a place */
    if (value < 1 || value > 64) return fail(WGA_E_INVALID_ARG, "stat_pair_hash_bits: 1 .. 64", nullptr);
    c->stat_pair_hash_bits = (unsigned)value;
    return WGA_OK;
  }
  if (strcmp(name, "maf_index_sort_bits") == 0) { /* wga_maf_index: the digit width of its sort by group */
    if (value < 1 || value > (int64_t)WGA_SORT_MAX_BITS) return fail(WGA_E_INVALID_ARG, "maf_index_sort_bits: 1 .. 8", nullptr);
    c->maf_index_sort_bits = (unsigned)value;
    return WGA_OK;
  }
  if (strcmp(name, "expand_variant") == 0) {
    if (value != -1 && value != 0 && value != 3) return fail(WGA_E_INVALID_ARG, "expand_variant: -1 (the library's choice), 0, 3", nullptr);
    c->expand_variant = (int)value;
    return WGA_OK;
  }
  if (strcmp(name, "expand_job_tiles") == 0) { /* streaming row kernel: consecutive tiles per wave */
    if (value < 0 || value > (int64_t)WGA_S_MAX_JOB_TILES) return fail(WGA_E_INVALID_ARG, "expand_job_tiles: 0 (by the batch), 1 .. 32", nullptr);
    c->expand_job_tiles = (int)value;
    return WGA_OK;
  }
  if (strcmp(name, "pseudo_variant") == 0) { /* wga_pafpseudo_fill: 3 the streaming row kernel (default), 0 one block per tile */
    if (value != 0 && value != 3) return fail(WGA_E_INVALID_ARG, "pseudo_variant: 0, 3", nullptr);
    c->pseudo_variant = (int)value;
    return WGA_OK;
  }
  if (strcmp(name, "expand_timing") == 0) {
    if (value && !c->timing) {
      int rc = ctx_bind(c);
      if (rc) return rc;
      for (int k = 0; k < 2 * wga_ctx::kTimingRing; k++) {
        const char* e = rt_event_create(&c->ev[k]);
        if (e) { /* give back what was created: `timing` stays off, nobody else would destroy them */
          for (int j = 0; j < k; j++) rt_event_destroy(c->ev[j]);
          return fail(WGA_E_HIP, "rt_event_create", e);
        }
      }
    }
    if (!value && c->timing)
      for (int k = 0; k < 2 * wga_ctx::kTimingRing; k++) rt_event_destroy(c->ev[k]);
    c->timing = value != 0;
    c->ev_n = 0;
    return WGA_OK;
  }
  return fail(WGA_E_INVALID_ARG, "unknown parameter", name);
}

int wga_sync(wga_ctx* c) {
  int rc = ctx_bind(c);
  if (rc) return rc;
  RT_CHECK(rt_sync(c->stream));
  return WGA_OK;
}
int wga_malloc(wga_ctx* c, size_t bytes, void** d_out) {
  int rc = ctx_bind(c);
  if (rc) return rc;
  if (!d_out) return fail(WGA_E_INVALID_ARG, "d_out is null", nullptr);
  const char* e = rt_malloc(d_out, bytes);
  if (e) return fail(WGA_E_OOM, "device allocation", e);
  return WGA_OK;
}
/* What a count call left for its fill call (the K11 scan, the piece tables of K3 / K4 and of K7 / K10 / K12, pafpseudo's class
 * sums) is keyed by the arrays it was made from.  Writing into one of those arrays through the library, or freeing it, drops it:
 * a fill call then computes its own.  [lo, lo + bytes) is the range written (bytes == 0: the allocation that starts at lo). */
static void ctx_arrays_written(wga_ctx* c, const void* lo, size_t bytes) {
  for (CallCache* k : {&c->maf_cache, &c->op_tab.cache, &c->elem_scan.cache, &c->class_tab.cache}) k->written(lo, bytes);
}

int wga_free(wga_ctx* c, void* d_ptr) {
  int rc = ctx_bind(c);
  if (rc) return rc;
  if (d_ptr) ctx_arrays_written(c, d_ptr, 0); /* what a count call left for its fill call does not outlive the arrays it was made from */
  if (d_ptr) RT_CHECK(rt_free(d_ptr));
  return WGA_OK;
}
int wga_memcpy_h2d(wga_ctx* c, void* d_dst, const void* h_src, size_t bytes) {
  int rc = ctx_bind(c);
  if (rc) return rc;
  if (bytes) {
    ctx_arrays_written(c, d_dst, bytes);
    RT_CHECK(rt_h2d(d_dst, h_src, bytes, c->stream));
  }
  return WGA_OK;
}
int wga_memcpy_d2h(wga_ctx* c, void* h_dst, const void* d_src, size_t bytes) {
  int rc = ctx_bind(c);
  if (rc) return rc;
  if (bytes)
    RT_CHECK(rt_d2h(h_dst, d_src, bytes, c->stream));
  else
    RT_CHECK(rt_sync(c->stream));
  return WGA_OK;
}
int wga_host_alloc(wga_ctx* c, size_t bytes, void** h_out) {
  int rc = ctx_bind(c);
  if (rc) return rc;
  if (!h_out) return fail(WGA_E_INVALID_ARG, "h_out is null", nullptr);
  const char* e = rt_host_alloc(h_out, bytes);
  if (e) return fail(WGA_E_OOM, "pinned host allocation", e);
  return WGA_OK;
}
int wga_host_free(wga_ctx* c, void* h_ptr) {
  int rc = ctx_bind(c);
  if (rc) return rc;
  if (h_ptr) RT_CHECK(rt_host_free(h_ptr));
  return WGA_OK;
}
int wga_memcpy_d2h_async(wga_ctx* c, void* h_dst, const void* d_src, size_t bytes) {
  int rc = ctx_bind(c);
  if (rc) return rc;
  if (bytes) RT_CHECK(rt_d2h_async(h_dst, d_src, bytes, c->stream));
  return WGA_OK;
}
int wga_memset(wga_ctx* c, void* d_dst, int byte, size_t bytes) {
  int rc = ctx_bind(c);
  if (rc) return rc;
  if (bytes) {
    ctx_arrays_written(c, d_dst, bytes);
    RT_CHECK(rt_memset(d_dst, byte, bytes, c->stream));
  }
  return WGA_OK;
}

int wga_ctx_get_param(wga_ctx* c, const char* name, int64_t* value) {
  if (!c || !name || !value) return fail(WGA_E_INVALID_ARG, "null argument", nullptr);
  if (strcmp(name, "cov_spin_limit") == 0) {
    *value = (int64_t)c->cov_spin_limit;
    return WGA_OK;
  }
  if (strcmp(name, "expand_drain_min") == 0) { /* what the last wga_paf2maf_expand used */
    *value = (int64_t)c->expand_drain_min_used;
    return WGA_OK;
  }
  if (strcmp(name, "expand_variant") == 0) {
    *value = (int64_t)c->expand_variant;
    return WGA_OK;
  }
  if (strcmp(name, "expand_stream_left_to_v1") == 0) { /* tiles the streaming kernel's last launch left to v1 (a device read: diagnostics) */
    *value = c->expand_variant_used == 3 ? -1 : 0; /* -1: the scratch that held the counters has been handed on */
    if (c->expand_variant_used == 3 && c->stream_counts) {
      u32 h[2] = {0, 0};
      int rc = ctx_bind(c);
      if (rc) return rc;
      RT_CHECK(rt_d2h(h, c->stream_counts, sizeof(h), c->stream));
      *value = (int64_t)h[0] + (int64_t)h[1];
    }
    return WGA_OK;
  }
  if (strcmp(name, "paf_pair_hash_bits") == 0) {
    *value = (int64_t)c->paf_pair_hash_bits;
    return WGA_OK;
  }
  if (strcmp(name, "maf_index_hash_bits") == 0) {
    *value = (int64_t)c->maf_index_hash_bits;
    return WGA_OK;
  }
  if (strcmp(name, "maf_index_sort_bits") == 0) {
    *value = (int64_t)c->maf_index_sort_bits;
    return WGA_OK;
  }
  if (strcmp(name, "stat_pair_hash_bits") == 0) {
    *value = (int64_t)c->stat_pair_hash_bits;
    return WGA_OK;
  }
  if (strcmp(name, "expand_job_tiles") == 0) {
    *value = (int64_t)c->expand_job_tiles;
    return WGA_OK;
  }
  if (strcmp(name, "pseudo_variant") == 0) {
    *value = (int64_t)c->pseudo_variant;
    return WGA_OK;
  }
  if (strcmp(name, "pseudo_stream_left_to_blocks") == 0) { /* tiles the last base-mode wga_pafpseudo_fill left to the block kernel */
    *value = -1; /* not known (no such launch yet, or the scratch that held the counters has been handed on) */
    if (c->pseudo_counts) {
      u32 h[2] = {0, 0};
      int rc = ctx_bind(c);
      if (rc) return rc;
      RT_CHECK(rt_d2h(h, c->pseudo_counts, sizeof(h), c->stream));
      *value = (int64_t)h[0] + (int64_t)h[1];
    }
    return WGA_OK;
  }
  if (strcmp(name, "expand_variant_used") == 0) { /* what the last wga_paf2maf_expand ran */
    *value = (int64_t)c->expand_variant_used;
    return WGA_OK;
  }
  return fail(WGA_E_INVALID_ARG, "unknown parameter", name);
}

} /* extern "C" */

/* the launchers, one part per kernel family (job_tiles_for of the first is also pafpseudo's) */
#include "capi_paf2maf.inc"
#include "capi_maf.inc"
#include "capi_opwalk.inc"
#include "capi_text.inc"
#include "capi_paf_fix.inc"
#include "capi_chain_write.inc"
#include "capi_chain2paf.inc"
#include "capi_maf2paf.inc"
#include "capi_chain_heads.inc"
#include "capi_pafpseudo_frame.inc"
#include "capi_maf_frame.inc"
#include "capi_stat_rows.inc"
#include "capi_dotplot_overview.inc"
#include "capi_dotplot_csv.inc"
#include "capi_maf_index.inc"
#include "capi_stat_pairs.inc"
#include "capi_pafcov.inc"
#include "capi_pafpseudo.inc"
#include "capi_multigpu.inc"
