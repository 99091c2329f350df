/*
 * wga_hip.h — C-ABI of libwgahip.so: the MI355X (gfx950) engine for wgatools' CIGAR-driven hot path.
 *
 * Every compute entry point replaces one per-record Rust function of the reference (cited per
 * function as /root/reference-relative file:line) with a *batched* call over many records.
 *
 * Conventions
 *   - plain C, no ownership transfer: the caller allocates every input and output buffer.
 *   - every `const T* d_*` / `T* d_*` argument is a DEVICE pointer (HBM resident).  Callers that
 *     do not link HIP themselves (a Rust/cgo/ctypes binding) use wga_malloc/wga_memcpy_* below.
 *   - `d_ops` must be 16-byte aligned (hipMalloc / wga_malloc guarantee 256).
 *   - calls are asynchronous on the context's stream; wga_sync() (or a D2H copy) waits.
 *   - return value: 0 = WGA_OK, negative = wga_status.  Per-record problems never fail the call:
 *     they are reported in `wga_rec_diag` so the host can print the reference's message for the
 *     first failing record in input order (reference: errors.rs:45-74, main.rs:14-21).
 *
 * Packed CIGAR op (u32): len << 4 | code, len < 2^28.  Codes follow BAM for the nine standard
 * ops; the packer (wga_cigar_pack) splits longer lengths into several ops and marks the pieces of
 * a split I / D with continuation codes so that event counts stay exact.
 */
#ifndef WGA_HIP_H
#define WGA_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 2: what a count call leaves in the context for its fill call (wga_maf_runs_* / wga_chain_lines_*, the op walks
 *    wga_paf_call_events / wga_cigar_chain / wga_cigar_dotplot over long records, wga_cigar_class_sums -> wga_pafpseudo_fill)
 *    is ONE-SHOT — the first fill call that takes it consumes it — and is dropped when one of the arrays it was made from is
 *    written through wga_memcpy_h2d / wga_memset or freed; "expand_variant" takes -1, 0, 2, 3.
 * 3: the output-placement calls (wga_paf2maf_expand_place, wga_arena_alloc, wga_arena_probe) and the parameters
 *    "expand_autotune" / "expand_alias" are gone — the streaming row kernel made them unnecessary —; new:
 *    wga_pafcov_accumulate_final; wga_reduce_scatter_i32 no longer waits on the host (its result is ordered on the contexts'
 *    streams) and wga_pafcov_finalize refuses overlapping target ranges.  No struct layout changed. */
#define WGA_ABI_VERSION 3

/* The contract of every two-call protocol (count call, then fill call; also wga_maf_pair_stat / wga_maf_call_runs, whose count
 * call leaves the table of its long blocks): the input arrays of a count call must not be rewritten outside the library before
 * its fill call.  The context recognises the fill call by the arrays' addresses, the counts and the parameters — every input
 * array of the call, the strand array included —, not by their contents.  Writes through wga_memcpy_h2d / wga_memset and a
 * wga_free are seen and drop what was kept; a kernel or copy of the caller's own is not: fence it with a new count call. */

/* ---- status codes (call level) ------------------------------------------------------------ */
enum wga_status {
  WGA_OK = 0,
  WGA_E_INVALID_ARG = -1,
  WGA_E_NO_DEVICE = -2,
  WGA_E_HIP = -3, /* a HIP runtime call failed; see wga_last_error() */
  WGA_E_OOM = -4,
  WGA_E_TOO_SMALL = -5, /* caller buffer too small (host packer) */
  WGA_E_FALLBACK = -6   /* wga_maf_index: the line table holds a WGA_MAF_FALLBACK line, the piece is the host reader's */
};

/* ---- packed op codes ---------------------------------------------------------------------- */
enum wga_op_code {
  WGA_OP_M = 0,
  WGA_OP_I = 1,
  WGA_OP_D = 2,
  WGA_OP_N = 3,
  WGA_OP_S = 4,
  WGA_OP_H = 5,
  WGA_OP_P = 6,
  WGA_OP_EQ = 7,
  WGA_OP_X = 8,
  WGA_OP_I_CONT = 9,   /* continuation of a split I: same bases, no new event */
  WGA_OP_D_CONT = 10,  /* continuation of a split D */
  WGA_OP_OTHER = 11    /* any other single-char op (`B`, `z`, `é`, ...): the reference accepts the
                          token and lets each consumer decide (cigar.rs:43-56) */
};
#define WGA_OP_LEN_BITS 28
#define WGA_OP_MAX_LEN ((1u << WGA_OP_LEN_BITS) - 1u)
#define WGA_PACK_OP(len, code) (((uint32_t)(len) << 4) | (uint32_t)(code))

/* ---- per-record error codes: 1:1 with the WGAError variants the hot path can raise --------- */
enum wga_rec_err {
  WGA_REC_OK = 0,
  WGA_REC_CIGAR_TAG_NOT_FOUND = 1, /* errors.rs:57  "CIGAR start tag not found"            */
  WGA_REC_CIGAR_OP_INVALID = 2,    /* errors.rs:59  "CIGAR OP `{0}` invalid"               */
  WGA_REC_PARSE_INT = 3,           /* errors.rs:51  "Parse `{0}` Into Integer Error"       */
  WGA_REC_INVALID_BASE = 4,        /* errors.rs:73  "Invalid Base: `{0}`"                  */
  WGA_REC_NOM = 5,                 /* errors.rs:45  nom tag error                          */
  WGA_REC_PANIC = 6                /* the reference panics (errors.rs:92 slice, String::insert_str
                                      out of range at cigar.rs:507,513)                    */
};

#define WGA_NONE UINT64_MAX

/* Device-side per-record diagnostics (all fields WGA_NONE when clean).  Written with atomicMin so
 * "first in op order" / "first in reversed-sequence order" is exact. */
typedef struct {
  uint64_t bad_op_idx;   /* first op (index inside the record) the consumer rejects              */
  uint64_t panic_op_idx; /* first I/D op whose insertion point lies beyond the fetched sequence  */
  uint64_t bad_base_pos; /* first invalid base in reverse-complement order (utils.rs:85-98)      */
} wga_rec_diag;

/* = struct Cigar sans text (cigar.rs:16-29) */
typedef struct {
  uint64_t match, mismatch, ins_ev, ins_bp, del_ev, del_bp, inv_ins_ev, inv_ins_bp, inv_del_ev,
      inv_del_bp, inv_ev;
} wga_cigar_counts;

/* CSR batch of n records: d_ops[d_op_off[i] .. d_op_off[i+1]) belong to record i. */
typedef struct {
  const uint32_t* d_ops;
  const uint64_t* d_op_off; /* n+1 entries, d_op_off[0] == 0 */
  const uint8_t* d_strand_neg; /* n entries, 1 = '-' (common.rs:42-48) */
  uint64_t n_ops;              /* == d_op_off[n] (host copy, sizes the launch) */
  uint32_t n;
} wga_cigar_batch;

typedef struct wga_ctx wga_ctx;

/* ---- context / runtime plumbing ------------------------------------------------------------ */
int wga_abi_version(void);
const char* wga_last_error(void);
int wga_device_count(void);
/* THREADING / STREAM CONTRACT.  A context belongs to ONE host thread at a time and orders all its work on ONE
 * stream: its scratch arenas (scan partials, descriptors, coverage piece lists) are shared by every entry point and
 * reused from call to call, which is only safe because calls are stream-ordered.  Use one context per host thread /
 * per device; wga_ctx_set_stream / wga_ctx_reset_stream drain the stream they leave before switching.
 * wga_ctx_destroy waits for the context's stream. */
int wga_ctx_create(int device, wga_ctx** out);
void wga_ctx_destroy(wga_ctx*);
/* Launch on an external stream (a hipStream_t, e.g. torch.cuda.current_stream().cuda_stream;
 * NULL is HIP's default stream).  wga_ctx_reset_stream goes back to the context's own stream.  Both
 * synchronise the stream that is being left: an external stream must stay alive until the next
 * wga_ctx_set_stream / wga_ctx_reset_stream / wga_ctx_destroy on the context. */
int wga_ctx_set_stream(wga_ctx*, void* hip_stream);
int wga_ctx_reset_stream(wga_ctx*);
/* Tunables (test knobs): "expand_force_slow" (0/1) forces the u64 op-serial fallback of the
 * expand kernel; "expand_no_table" (0/1) forces its binary-search event lookup; "expand_variant" picks the row
 * kernel — same bytes either way: -1 (default) or 3: the streaming kernel, one wave per row kind of a run of tiles
 * (profiles/r04_k2s_experiments.md), 0: v1 (one block per tile; also the kernel of the tiles the streaming kernel leaves).  The
 * window kernel of rounds 3-5 (2) was retired in round 6: it was ahead only for batches below 100 ops per record
 * kernel (environment: WGA_EXPAND_VARIANT); "expand_job_tiles" (1 .. 32; 0, the default: 8, or 4 for batches below 200 000 tiles): consecutive tiles one wave of the
 * streaming kernel walks;
 * "pseudo_variant": wga_pafpseudo_fill's rows through the streaming kernel (3, default) or one block per tile (0);
 * "expand_drain_min" (0 .. 64, v1 only) = how many gap-touching 16-column chunks a wave
 * queues before it emits them: 0 (default) lets the library choose by the size of the two sequence pools — 32 when
 * they stay in the 256 MB Infinity Cache, 16 when they do not (environment: WGA_EXPAND_DRAIN_MIN).
 * "reduce_same_device_ok" / "reduce_staged" (0/1): wga_reduce_scatter_i32 over contexts that share a device, and by staged
 * peer copies where peer access exists (tests on one-GPU boxes).
 * "cov_spin_limit" (default 4096): wga_pafcov_accumulate's list pass polls a tile sum this often before it adds up the ops itself.
 * "op_long_ops" (default 16384) / "op_piece_ops" (8192, a multiple of 256): the op walks with one wave per record (call
 * events, chain lines, dotplot segments) cut records beyond the first into pieces of at most the second and walk the pieces
 * over the whole chip; "maf_long_cols" (32768; 61440 at most: longer blocks are long whatever it says) / "maf_piece_cols"
 * (16384): the same for the MAF column walks — a long block is listed, planned and walked in pieces on the device (no
 * read-back); when the configured piece size would make more than 32 768 pieces beyond one per long block, the piece grows
 * to whole steps of 2 048 columns that stay inside that budget.  "maf_group" (0 .. 8, default 0 = by the number of blocks:
 * n / 24 576, at least 1, at most 8): consecutive MAF blocks one wave walks as one column stream.  The tests set small values
 * to reach those paths with small inputs. */
int wga_ctx_set_param(wga_ctx*, const char* name, int64_t value);
/* Read back: "cov_spin_limit" (the setting), "expand_drain_min" = what the last wga_paf2maf_expand used,
 * "expand_variant" / "expand_job_tiles" / "pseudo_variant" (the settings), "expand_variant_used" (what the last
 * wga_paf2maf_expand ran), "expand_stream_left_to_v1" / "pseudo_stream_left_to_blocks" (tiles the streaming kernel's last
 * launch left to the block kernels: records whose slices do not match their CIGAR, slices at a pool's edge, giant tiles —
 * a device read, diagnostics; -1 once another call has taken the scratch arena the two counters lay in). */
int wga_ctx_get_param(wga_ctx*, const char* name, int64_t* value);
/* Measurement hook: after wga_ctx_set_param(ctx, "expand_timing", 1) every wga_paf2maf_expand
 * brackets its gap-insertion kernel (without the descriptor pre-pass) with two events on the
 * launch stream.  Returns the summed kernel time of the launches since the last call (at most the
 * 64 most recent) and their number; waits for them. */
int wga_ctx_expand_timing(wga_ctx*, double* ms_sum, uint32_t* launches);
int wga_sync(wga_ctx*);
int wga_malloc(wga_ctx*, size_t bytes, void** d_out);
int wga_free(wga_ctx*, void* d_ptr);
int wga_memcpy_h2d(wga_ctx*, void* d_dst, const void* h_src, size_t bytes);
int wga_memcpy_d2h(wga_ctx*, void* h_dst, const void* d_src, size_t bytes); /* synchronises */
int wga_memset(wga_ctx*, void* d_dst, int byte, size_t bytes);
/* Pinned host memory and an asynchronous device-to-host copy on the context's stream: what a writer needs to stream
 * a result (the MAF text of converter.rs:237-262, the BED lines of pafcov.rs:56-60) out of HBM in pieces while the
 * next piece is copied — wga_sync (or a later synchronising call) before the host reads h_dst. */
int wga_host_alloc(wga_ctx*, size_t bytes, void** h_out);
int wga_host_free(wga_ctx*, void* h_ptr);
int wga_memcpy_d2h_async(wga_ctx*, void* h_dst, const void* d_src, size_t bytes);

/* ---- host: CIGAR text -> packed ops (replaces the nom tokeniser, cigar.rs:43-75,
 *      utils.rs:69-74; driven per record by every consumer, e.g. cigar.rs:529-549) ------------
 * `text` is the CIGAR *after* the "cg:Z:" tag.  Emits ops until the first tokeniser error, which
 * is returned in *err (wga_rec_err) with the offending token in [*err_tok_off, +*err_tok_len).
 * Returns WGA_OK, or WGA_E_TOO_SMALL with *n_ops = required capacity. */
int wga_cigar_pack(const char* text, size_t len, uint32_t* ops, size_t cap, size_t* n_ops,
                   int32_t* err, size_t* err_tok_off, size_t* err_tok_len);
/* Upper bound of ops wga_cigar_pack can emit for `len` bytes of text. */
size_t wga_cigar_pack_bound(const char* text, size_t len);

/* ---- device tokeniser: the same text -> packed ops conversion as wga_cigar_pack, for callers that
 *      keep the CIGAR text on the device (the host tokeniser is the floor of
 *      every end-to-end run).  Record i's text (after the tag) is d_text[d_text_off[i] ..
 *      d_text_off[i+1]).  Two calls: with d_ops == NULL it fills d_op_cnt[n] (ops the record packs
 *      to, up to its first tokeniser error) and d_err[n]; after an exclusive scan of the counts the
 *      second call writes the ops at d_ops + d_op_off[i].  Error codes, token offsets and the
 *      splitting of lengths >= 2^28 are those of wga_cigar_pack. */
typedef struct {
  int32_t err;      /* wga_rec_err */
  uint32_t tok_len; /* offending token inside the record's text: length ... */
  uint64_t tok_off; /* ... and offset */
} wga_tok_err;
int wga_cigar_tokenise(wga_ctx*, uint32_t n, const uint8_t* d_text, const uint64_t* d_text_off,
                       uint64_t* d_op_cnt, wga_tok_err* d_err, uint32_t* d_ops,
                       const uint64_t* d_op_off);

/* ---- K1: PAF stat walk (replaces parse_paf_to_cigar, cigar.rs:629-707) ----------------------
 * d_counts[n]; d_diag[n] (bad_op_idx set for ops other than M = X I D).
 * d_tile_ws (optional, may be NULL): wga_tile_ws_bytes(n_ops) bytes, filled with the per-tile
 * partial sums wga_paf2maf_expand needs to place a tile inside a long record. */
size_t wga_tile_ws_bytes(uint64_t n_ops);
int wga_cigar_stat(wga_ctx*, const wga_cigar_batch*, wga_cigar_counts* d_counts,
                   wga_rec_diag* d_diag, void* d_tile_ws);

/* ---- paf2maf row geometry (host logic of converter.rs:196-263 moved on device) --------------
 * Row lengths follow String::insert_str semantics: t_row_len = t_src_len + I bases,
 * q_row_len = q_src_len + D bases (cigar.rs:504-515).  Each record occupies
 *   pre_t[i] | t row | pre_q[i] | q row | post[i]   bytes of the output text
 * (pre/post = the MAF line text around the rows, maf.rs:566-581; NULL = 0).
 * Outputs: d_t_row_off[n], d_q_row_off[n], d_rec_off[n+1] (d_rec_off[n] = total bytes). */
int wga_paf2maf_layout(wga_ctx*, uint32_t n, const wga_cigar_counts* d_counts,
                       const uint64_t* d_t_src_len, const uint64_t* d_q_src_len,
                       const uint32_t* d_pre_t, const uint32_t* d_pre_q, const uint32_t* d_post,
                       uint64_t* d_t_row_off, uint64_t* d_q_row_off, uint64_t* d_rec_off);

/* ---- K2: paf2maf gap insertion (replaces parse_cigar_to_insert + cigar_unit_insert_seq,
 *      cigar.rs:492-551, and reverse_complement, utils.rs:83-101) -----------------------------
 * t_fa/q_fa: ungapped forward-strand sequence pools; record i uses
 *   t_fa[t_src_off[i] .. +t_src_len[i])   and   q_fa[q_src_off[i] .. +q_src_len[i])
 * (what faidx fetch returned, converter.rs:219-225).  For strand '-' the kernel reads the query
 * slice reversed and complemented.  Writes the two gapped rows at d_out + d_*_row_off[i].
 * d_counts / d_tile_ws must come from wga_cigar_stat on the same batch; d_diag is updated
 * (panic_op_idx, bad_base_pos). */
int wga_paf2maf_expand(wga_ctx*, const wga_cigar_batch*, const wga_cigar_counts* d_counts,
                       const void* d_tile_ws, const uint8_t* d_t_fa, uint64_t t_fa_bytes,
                       const uint64_t* d_t_src_off, const uint64_t* d_t_src_len,
                       const uint8_t* d_q_fa, uint64_t q_fa_bytes, const uint64_t* d_q_src_off,
                       const uint64_t* d_q_src_len, uint8_t* d_out, const uint64_t* d_t_row_off,
                       const uint64_t* d_q_row_off, wga_rec_diag* d_diag);

/* Copy n variable-length byte snippets: d_dst[d_dst_off[i] ..) = d_src[d_src_off[i] .. d_src_off[i+1])
 * (used to drop the "a score=…" / "s\tname\t…" line text between the rows, maf.rs:566-581). */
int wga_scatter_bytes(wga_ctx*, uint32_t n, const uint8_t* d_src, const uint64_t* d_src_off,
                      uint8_t* d_dst, const uint64_t* d_dst_off);

/* ---- K3: MAF column-pair walk (replaces parse_maf_seq_to_cigar + cigar_cat_ext,
 *      cigar.rs:298-308,344-432) ---------------------------------------------------------------
 * Record i compares d_rows[t_off[i] + j] with d_rows[q_off[i] + j] for j < cols[i]
 * (cols = min of the two row lengths: `zip` truncates).  d_counts[n] as K1.
 * Optional run list for maf2paf's cg:Z: text (maf.rs:484-520): d_run_cnt[n] always receives the
 * number of runs of record i; if d_runs != NULL record i's runs are written in order to
 * d_runs[d_run_off[i] ..) as (start_column << 3 | class), class 0 '=', 1 'I', 2 'D', 3 'X'
 * (a run's length is the next run's start — or cols[i] — minus its own start).  Call once with
 * d_runs == NULL to size, scan d_run_cnt (wga_exclusive_scan_u64), call again. */
int wga_maf_pair_stat(wga_ctx*, uint32_t n, const uint8_t* d_rows, const uint64_t* d_t_off,
                      const uint64_t* d_q_off, const uint64_t* d_cols,
                      const uint8_t* d_strand_neg, wga_cigar_counts* d_counts,
                      uint64_t* d_run_cnt, uint64_t* d_runs, const uint64_t* d_run_off);

/* ---- K4: MAF call column walk (replaces the group_by(cigar_cat_ext_caller) scan of
 *      call_within_var, caller.rs:444-446, and the per-column gap scans of
 *      find_safe_chunk_boundary :173-199 / create_chunk_record :240-251) -------------------------
 * Ordered list of maximal runs of equal caller class per record (cigar.rs:314-328), 3 u64 per
 * run: [0] start_column << 3 | class (0 '=', 1 I, 2 D, 3 X, 4 W = both rows gapped),
 * [1] non-gap target characters before the run, [2] non-gap query characters before it.
 * Same two-call protocol as wga_maf_pair_stat (d_runs == NULL sizes; d_run_off counts runs). */
int wga_maf_call_runs(wga_ctx*, uint32_t n, const uint8_t* d_rows, const uint64_t* d_t_off,
                      const uint64_t* d_q_off, const uint64_t* d_cols, uint64_t* d_run_cnt,
                      uint64_t* d_runs, const uint64_t* d_run_off);

/* ---- call on PAF: the op walk (replaces the fold of call_within_var_paf, caller.rs:664-819) ---
 * Walks each record's ops with the running target / query positions and the `after_m` flag of
 * the reference and lists the ops that raise VCF rows: every X op when `snp` is set (one row per
 * column, :688-717), and every I / D op that directly follows an M / = / X op and is longer than
 * `svlen` (:719-813).  The walk of a record stops at its first op outside M = X I D (the
 * reference's fold keeps the CigarOpInvalid in its accumulator, skips the remaining ops and then
 * discards the error, :673,815-819).  An I / D whose length was split by the packer (>= 2^28) is
 * listed when a continuation piece follows; the caller applies the cutoff to the summed length.
 * Event = 3 u64: op index within the record, target bases before the op, query bases before it
 * (both relative to the record's start coordinates).  Same two-call protocol as wga_maf_call_runs:
 * d_ev == NULL -> only d_ev_cnt[n]; then d_ev_off = exclusive scan and the call again. */
int wga_paf_call_events(wga_ctx*, const wga_cigar_batch*, uint64_t svlen, int snp, uint64_t* d_ev_cnt,
                        uint64_t* d_ev, const uint64_t* d_ev_off);

/* ---- call on PAF: the VCF rows of the events (replaces the record building and printing of call_within_var_paf,
 *      caller.rs:640-658 the <INV> row of a '-' record, :688-717 one row per column of an X op, :719-813 the INS / DEL
 *      rows of indels longer than `svlen`; text layout of noodles-vcf 0.43, README.md:323-343) ---------------------
 * Record i's text is its rows in the reference's order:
 *   <target>\t<pos>\t.\t<REF>\t<ALT>\t.\t.\t<INFO or .>\tGT:QI\t1|1:<query>@<a>[@<b>]@<P|N>\n
 * d_ev / d_ev_off: the events of wga_paf_call_events on the same batch (with the same svlen).  d_recs: per record its
 * names (offsets into d_names), PAF coordinates and the place of its fetched target / query sequence inside the pools
 * (paf.rs:221-237: [start, end] inclusive, clipped at the contig end).  Two calls: d_out == NULL -> d_nbytes[n] and
 * d_err[n]; then d_out_off = exclusive scan of d_nbytes and the call again with d_out.  d_err[i].item == ~0: clean
 * (kind and ch are 0); otherwise the record's first failing item (0 = the <INV> row, 1 + e = event e) with kind 1 = a
 * REF / ALT slice outside the fetched sequence (the reference's slice panic, caller.rs:695-696,753-754,800-801) or
 * kind 2 = a base outside ACGTN in any case (noodles-vcf's parse error; ch = the byte); the record's text ends in front
 * of that item.  A '-' record whose fetched target is empty (t_len == 0) reports kind 1 at item 0 (the <INV> row quotes
 * the first fetched base, :642) and has no text: the kernel reads no byte of a sequence whose length is 0, and t_off /
 * q_off only have to lie inside the pools.  An indel event in front of which neither sequence has advanced (a
 * zero-length M-like op: `0=5I`) is kind 1 as well (the reference's slice start underflows, :733-737,786-790).  The fill
 * pass writes record i's d_nbytes[i] bytes into [d_out_off[i], d_out_off[i + 1]) and touches no other byte of d_out. */
typedef struct {
  uint64_t t_name_off, q_name_off;
  uint32_t t_name_len, q_name_len;
  uint64_t t_start, t_end, q_start, q_end;
  uint64_t t_off, t_len, q_off, q_len;
} wga_vcf_rec;
typedef struct {
  uint64_t item;
  uint32_t kind, ch;
} wga_vcf_err;
int wga_paf_call_vcf(wga_ctx*, const wga_cigar_batch*, uint64_t svlen, const uint64_t* d_ev, const uint64_t* d_ev_off,
                     const wga_vcf_rec* d_recs, const uint8_t* d_names, const uint8_t* d_t_pool,
                     const uint8_t* d_q_pool, uint64_t* d_nbytes, wga_vcf_err* d_err, uint8_t* d_out,
                     const uint64_t* d_out_off);

/* ---- call on MAF: chunk cuts, event rules and VCF rows on the run list (replaces find_safe_chunk_boundary
 *      caller.rs:159-219, create_chunk_record :221-265 and the fold + record building of call_within_var :388-608;
 *      text layout of noodles-vcf 0.43, README.md:323-343) ---------------------------------------------------------
 * d_rows / d_t_off / d_q_off / d_cols / d_runs / d_run_off: the arrays of wga_maf_call_runs (cols = the target row's
 * length, caller.rs:115) and the run list it wrote.  d_recs: per block its names (offsets into d_names), the two s lines'
 * start fields, the query's source size and strand (maf.rs:65-73).  Block i's text = the rows of its chunks in order: the
 * <INV> row of a '-' block's chunk (`inv`, :423-440), one row per column of an X run (`snp`, :570-603), one row per I / D
 * run longer than `svlen` that follows an '=' / X run (:464-569).  Two calls as wga_paf_call_vcf: d_out == NULL ->
 * d_nbytes[n], d_err[n] (item == ~0: clean; kind 2 = a REF / ALT base outside ACGTN in any case, ch = the byte:
 * noodles-vcf's parse error); then d_out_off = exclusive scan of d_nbytes and the call again with d_out.  A block's text
 * ends in front of the chunk that holds its first bad base (a chunk's records are collected before any is written, :137-141).
 * d_err[i].item of a bad block: only `!= ~0` is promised (today a count that goes on over the chunks' 64-run steps, not a run
 * index); kind and ch identify the error.  The fill pass writes block i's d_nbytes[i] bytes into
 * [d_out_off[i], d_out_off[i + 1]) and touches no other byte of d_out: d_out_off needs all n + 1 entries of the scan. */
typedef struct {
  uint64_t t_name_off, q_name_off;
  uint32_t t_name_len, q_name_len;
  uint64_t t_start, q_start, q_size;
  uint32_t q_neg, pad;
} wga_maf_vcf_rec;
int wga_maf_call_vcf(wga_ctx*, uint32_t n, const uint8_t* d_rows, const uint64_t* d_t_off, const uint64_t* d_q_off,
                     const uint64_t* d_cols, const uint64_t* d_runs, const uint64_t* d_run_off, const wga_maf_vcf_rec* d_recs,
                     const uint8_t* d_names, int snp, int inv, uint64_t svlen, uint64_t chunk_size, uint64_t* d_nbytes,
                     wga_vcf_err* d_err, uint8_t* d_out, const uint64_t* d_out_off);

/* ---- BGZF inflate on the device (the reference opens bgzipped FASTA through htslib's faidx,
 *      converter.rs:183-184, paf.rs:221-237, pseudomaf.rs:214-237) -------------------------------------------------
 * d_in: the compressed file as it is; d_blocks[n]: per BGZF member the place of its raw DEFLATE stream (behind the gzip
 * header with the BC field, in front of the CRC32 / ISIZE trailer), ISIZE and the place of its bytes in the output — the
 * host walks the member headers, nothing else.  Every block is inflated by one wave (RFC 1951: stored, fixed and dynamic
 * blocks) into d_out + out_off.  d_status[n]: 0, or the reason a stream is corrupt (WGA_INF_* in the kernel source: the
 * input ends inside a symbol, a bad block type / stored length, bad code lengths, an unused bit pattern, a distance in front
 * of the block, a size other than ISIZE); a corrupt block never writes outside its own out_len bytes.  The CRC32 of a
 * member is not part of its DEFLATE stream: wga_bgzf_crc32 computes it from the inflated bytes, for the caller to compare
 * with the member's trailer (the four bytes in front of ISIZE) as gzread and htslib do.
 *   wga_bgzf_crc32(d_text, n, d_blocks, d_crc)  d_crc[k] = CRC-32 of d_text[out_off .. out_off + out_len) of member k (one wave
 *                                               per member; in_off / in_len are not read; out_len < 2^29) */
typedef struct {
  uint64_t in_off;
  uint32_t in_len, out_len;
  uint64_t out_off;
} wga_bgzf_block;
int wga_bgzf_inflate(wga_ctx*, const uint8_t* d_in, uint64_t in_bytes, uint32_t n_blocks, const wga_bgzf_block* d_blocks,
                     uint8_t* d_out, uint32_t* d_status);
int wga_bgzf_crc32(wga_ctx*, const uint8_t* d_text, uint32_t n_blocks, const wga_bgzf_block* d_blocks, uint32_t* d_crc);

/* ---- paf2chain: the data lines of parse_cigar_to_chain + cigar_unit_chain
 *      (cigar.rs:251-295,460-490) and the head / tail indel trim of parse_cigar_to_trim
 *      (cigar.rs:202-245) that the chain header needs (chain.rs:142-183) ----------------------------
 * Record i's text is "\n<size>\t<dt>\t<dq>" per block but the last, then "\n<size>"; the caller puts
 * the header in front and "\n\n" behind (converter.rs:148-173).  Two calls: with d_out == NULL the
 * kernel fills d_trim[n], d_nbytes[n] (text bytes of record i) and d_diag[n].bad_op_idx (first op
 * outside M = X I D: CigarOpInvalid); the second call writes record i's text at d_out + d_out_off[i]. */
typedef struct {
  uint64_t head_ins, head_del, tail_ins, tail_del;
} wga_chain_trim_t;
int wga_cigar_chain(wga_ctx*, const wga_cigar_batch*, wga_chain_trim_t* d_trim, uint64_t* d_nbytes,
                    wga_rec_diag* d_diag, uint8_t* d_out, const uint64_t* d_out_off);

/* ---- K11: bridges between run / data-line lists, packed ops and CIGAR text ----
 * The remaining chain converters and maf2paf's text all reduce to walks that already exist once
 * their input is a wga_cigar_batch, and their CIGAR text is pure integer formatting:
 *   maf2chain  (converter.rs:57-91, parse_maf_seq_to_chain / _trim cigar.rs:155-199,435-457)
 *              = K3 runs -> wga_maf_runs_ops -> wga_cigar_chain  (cigar_cat merges '=' and X into M:
 *              cigar_unit_chain adds adjacent M-like ops into one size, cigar.rs:467-476)
 *   maf2paf    cg:Z: text (maf.rs:484-520, cigar.rs:400-401)          = wga_maf_runs_cigar_text
 *   chain2maf  (converter.rs:268-358, parse_chain_to_insert :360-388) = wga_chain_lines_ops -> K1 -> K2
 *   chain2paf  (chain.rs:430-452, parse_chain_to_cigar cigar.rs:554-627)
 *              = wga_chain_lines_ops -> K1 (matches, block length) + wga_chain_lines_cigar_text
 * A data line is three u64: size, 2nd text column (D bases), 3rd text column (I bases); a line is
 * walked as M size, I, D (zero lengths are left out of the ops; the text always has "<size>M").
 * Runs are K3's (wga_maf_pair_stat).  n_elems = d_*_off[n] = total runs / lines (< 2^32).
 * Two calls each: d_out == NULL fills d_cnt[n] (ops / bytes of record i); then record i's output is
 * written at d_out + d_out_off[i] (ops: in elements; text: in bytes).  The count call's scan of the
 * element sizes stays in the context for the fill call with the same arrays and counts (8 bytes per
 * element, grow-only).  It is one-shot (the fill call that takes it consumes it; a second fill call computes its own) and
 * is dropped when wga_free, wga_memcpy_h2d or wga_memset touches one of the arrays.  Contents changed behind the library's
 * back (another stream, another library) between the two calls are the caller's to fence with a new count call. */
int wga_maf_runs_ops(wga_ctx*, uint32_t n, uint64_t n_elems, const uint64_t* d_runs, const uint64_t* d_run_off,
                     const uint64_t* d_cols, uint64_t* d_cnt, uint32_t* d_out, const uint64_t* d_out_off);
int wga_maf_runs_cigar_text(wga_ctx*, uint32_t n, uint64_t n_elems, const uint64_t* d_runs,
                            const uint64_t* d_run_off, const uint64_t* d_cols, uint64_t* d_cnt, uint8_t* d_out,
                            const uint64_t* d_out_off);
int wga_chain_lines_ops(wga_ctx*, uint32_t n, uint64_t n_elems, const uint64_t* d_lines,
                        const uint64_t* d_line_off, uint64_t* d_cnt, uint32_t* d_out, const uint64_t* d_out_off);
int wga_chain_lines_cigar_text(wga_ctx*, uint32_t n, uint64_t n_elems, const uint64_t* d_lines,
                               const uint64_t* d_line_off, uint64_t* d_cnt, uint8_t* d_out,
                               const uint64_t* d_out_off);

/* ---- K12: dotplot base-level segments (replaces the fold over
 *      emit_baseplotdatas, cigar.rs:815-914, of parse_cigar_to_base_plotdata :917-952 and — on ops
 *      from wga_maf_runs_ops — parse_maf_to_base_plotdata :955-985) ----------------------------------
 * Per record the ordered BasePlotdata list (dotplot.rs:181-190) without the two names: 5 u64 per
 * segment = ref_start, ref_end, query_start, query_end (start / end swapped for '-' records as
 * reserve_query_start_end does), kind 0 'M' / 1 'I' / 2 'D'.  An I / D longer than `cutoff` is its
 * own segment; M-like ops and shorter indels merge into M segments; other ops are ignored.
 * d_t_start / d_q_start = target_start() / query_start() of the records.  Two calls: d_segs == NULL
 * fills d_seg_cnt[n]; then record i's segments go to d_segs + 5 * d_seg_off[i]. */
int wga_cigar_dotplot(wga_ctx*, const wga_cigar_batch*, uint64_t cutoff, const uint64_t* d_t_start,
                      const uint64_t* d_q_start, uint64_t* d_seg_cnt, uint64_t* d_segs,
                      const uint64_t* d_seg_off);

/* ---- K13: PAF field splitter (replaces the csv / serde record reader of
 *      paf.rs:24-30,50-78 and the tag lookup of get_cigar_string :122-141 for plain files) ---------
 * d_text = the PAF file as read (n_bytes < 4 GiB).  One wga_paf_line per text line, in order:
 * status WGA_PAF_OK (a record: the 12 fixed fields parsed like u64::from_str / Strand::from_str,
 * name spans and the span of the cg:Z: text as byte offsets into d_text — cg_beg == WGA_NONE when the
 * record has no cg:Z: tag), WGA_PAF_SKIP (blank line or '#' comment, which the csv reader drops) or
 * WGA_PAF_FALLBACK (a '"' or CR on the line, fewer than 12 fields, a field that does not parse, or
 * a cs:Z: tag standing in for cg:Z:): if any line says FALLBACK the caller must read the file with a
 * csv-semantics parser, which yields the same records or the reference's error text.
 * Two calls: d_lines == NULL returns *n_lines (host value; the call synchronises); then
 * d_lines[cap_lines >= *n_lines] is filled.  The cg spans feed wga_cigar_tokenise_spans, the
 * tokeniser on texts that are not back to back (record i = d_text[d_beg[i], d_end[i])). */
#define WGA_PAF_OK 0
#define WGA_PAF_SKIP 1
#define WGA_PAF_FALLBACK 2
typedef struct {
  uint64_t num[9]; /* query_length, query_start, query_end, target_length, target_start, target_end,
                      matches, block_length, mapq (paf.rs:50-65) */
  uint64_t qname_off, tname_off, cg_beg, cg_end;
  uint32_t qname_len, tname_len, n_fields;
  uint8_t strand_neg, status, pad[2];
} wga_paf_line;
int wga_paf_split(wga_ctx*, const uint8_t* d_text, uint64_t n_bytes, uint64_t* n_lines, wga_paf_line* d_lines,
                  uint64_t cap_lines);
int wga_cigar_tokenise_spans(wga_ctx*, uint32_t n, const uint8_t* d_text, const uint64_t* d_beg,
                             const uint64_t* d_end, uint64_t* d_op_cnt, wga_tok_err* d_err, uint32_t* d_ops,
                             const uint64_t* d_op_off);

/* ---- K14: MAF line splitter (replaces MAFReader / parse_sline for plain files, maf.rs:25-36,138-211,
 *      371-421; with it the K3 / K4 walks read the rows straight out of the uploaded file) -----------
 * One wga_maf_line per text line: WGA_MAF_SLINE (a line starting with 's' other than the file's first
 * line, split at white space into mode, name, start, size, strand, srcSize, text: numbers parsed like
 * u64::from_str / Strand::from_str, name and text as byte spans of d_text), WGA_MAF_OTHER (any other
 * line: it ends the block in progress) or WGA_MAF_FALLBACK (an s-line without exactly seven tokens,
 * with a field that does not parse or with a non-ASCII byte): the caller then reads the file with its
 * host reader, which returns the reference's error.  A block is a maximal run of s-lines.  Same
 * two-call protocol and size limit as wga_paf_split. */
#define WGA_MAF_SLINE 0
#define WGA_MAF_OTHER 1
#define WGA_MAF_FALLBACK 2
typedef struct {
  uint64_t num[3]; /* start, align_size, size (maf.rs:65-73) */
  uint64_t name_off, seq_off, seq_len;
  uint32_t name_len;
  uint8_t strand_neg, status, pad[2];
} wga_maf_line;
int wga_maf_split(wga_ctx*, const uint8_t* d_text, uint64_t n_bytes, uint64_t* n_lines, wga_maf_line* d_lines,
                  uint64_t cap_lines);

/* ---- K23: chain line splitter (replaces ChainRecords::next and the nom parsers chain_parser /
 *      parse_header / the data-line fold of chain.rs:58-73,206-383 for plain files) -------------------------------------
 * d_text = the chain file as read (n_bytes < 0xFFFFFFF0, 16 bytes of slack behind it).  Chain assembly happens on the device:
 * which lines are headers, a header's rank (= its chain index), the compaction of the data lines and what may follow what.
 *   d_heads[n_chains]       per chain: the eight header integers, the two strands, the two names as spans of d_text
 *   d_lines[3 * n_lines]    all data lines back to back: size, 2nd column, 3rd column (zeros for missing columns) — the
 *                           array wga_chain_lines_ops / wga_chain_lines_cigar_text take
 *   d_line_off[n_chains+1]  each chain's first data line
 * The file is taken (*status = WGA_CHAIN_OK) when all of this holds; otherwise *status = WGA_CHAIN_FALLBACK, *first_bad_line =
 * the index of the first line that breaks a rule (WGA_NONE when none does), and the caller reads the file with its nom-semantics
 * parser, which yields the same records or the reference's error text:
 *   - no CR and no byte >= 0x80 anywhere; a non-empty file ends in '\n' (nom drops an unterminated last data line)
 *   - every line is a header, a data line or empty; a line of white space only is not taken ("`size` Missing")
 *   - a header starts at column 0 with "chain" and a white-space byte ("chain1 t .." is a header for nom: left to the host) and
 *     has at least 12 more white-space separated tokens (surplus ones are ignored, chain.rs:206-322): the score is 1 to 15
 *     decimal digits (exact in an f64; any other float syntax is left to the host), the strands are "+" or "-", the eight
 *     integers parse like u64::from_str (optional '+', no overflow)
 *   - a data line has one to three tokens "+?digits" without overflow (a fourth, which nom ignores, is left to the host)
 *   - the first line is a header; a header is followed by a data line (header-header, header-blank and header-EOF are nom's
 *     Many1 error); a data line follows a header or a data line (nom skips one behind a blank line up to the next 'c'); a
 *     header may follow a data line directly; any number of blank lines may follow a chain's last data line
 *   - an empty file is taken: no chain
 * Two calls: with d_heads, d_lines and d_line_off all NULL the counts, the status and the first bad line are returned (host
 * values; the call synchronises); then the arrays (cap_chains >= *n_chains heads, cap_lines >= *n_data_lines triples) are
 * filled and the same host values returned.  With WGA_CHAIN_FALLBACK the arrays' contents mean nothing (the writes stay inside
 * the counted extents).  Workspace (context scratch, grow-only): 8 bytes per white-space byte and 8 per newline of the text, 16
 * bytes per byte of text at the most, plus 8 bytes per 256 lines. */
#define WGA_CHAIN_OK 0
#define WGA_CHAIN_FALLBACK 1
typedef struct {
  uint64_t num[8]; /* score, target_size, target_start, target_end, query_size, query_start, query_end, chain_id (chain.rs:76-91) */
  uint64_t tname_off, qname_off;
  uint32_t tname_len, qname_len;
  uint8_t tstrand_neg, qstrand_neg, pad[6];
} wga_chain_head;
int wga_chain_split(wga_ctx*, const uint8_t* d_text, uint64_t n_bytes, uint64_t* n_chains, uint64_t* n_data_lines,
                    uint32_t* status, uint64_t* first_bad_line, wga_chain_head* d_heads, uint64_t cap_chains,
                    uint64_t* d_lines, uint64_t cap_lines, uint64_t* d_line_off);
/* A run of chains [first, first + n) as a batch of its own for wga_chain_lines_ops / wga_chain_lines_cigar_text, which want
 * offsets that start at 0: d_out[i] = d_line_off[i] - d_line_off[0] for i = 0 .. n (pass d_line_off + first, and d_lines +
 * 3 * d_line_off[first] as the batch's lines).  d_out is another array than d_line_off. */
int wga_chain_line_off_rebase(wga_ctx*, uint32_t n, const uint64_t* d_line_off, uint64_t* d_out);

/* ---- stat totals: d_totals[11] = the column sums of d_counts[n] (wga_cigar_counts order).  What
 *      Statistic::merge adds up for one (ref, query) pair (stat.rs:181-223); with records sharded over
 *      GPUs these 88 bytes are the only thing `stat` has to all-reduce.  d_totals is overwritten. */
int wga_counts_total(wga_ctx*, uint32_t n, const wga_cigar_counts* d_counts, uint64_t* d_totals);

/* ---- FASTA text in HBM -> sequence pool (replaces the htslib faidx fetches of converter.rs:183-184,219-225,
 *      paf.rs:221-237, pseudomaf.rs:214-237: the drivers hand (contig, start, length) as an offset into the pool) ----
 * d_text = the FASTA file as read (decompressed if it was bgzf / gzip).  A header line starts with '>' at a line start;
 * the pool holds every byte of the sequence lines behind the first header, minus '\n' and a '\r' in front of one, case
 * preserved, contigs back to back in file order.  Two calls:
 *   d_pool == NULL: counts -> *n_contigs, *pool_bytes (host values; synchronises).
 *   otherwise     : fills d_pool[pool_bytes] and d_contigs[n_contigs]; a contig's name is the text behind '>' at
 *                   hdr_start up to the first white space (the host reads it from its own copy of the text).
 * Lookups keep htslib's semantics on the host side: first of duplicate names, end inclusive, clipped to the contig. */
typedef struct {
  uint64_t hdr_start; /* offset of the '>'                                          */
  uint64_t hdr_end;   /* offset of the header line's '\n' (n_bytes if the file ends) */
  uint64_t pool_off;  /* first base of the contig in the pool                        */
  uint64_t len;       /* bases                                                       */
} wga_fa_contig;
int wga_fasta_pool(wga_ctx*, const uint8_t* d_text, uint64_t n_bytes, uint64_t* n_contigs, uint64_t* pool_bytes,
                   uint8_t* d_pool, wga_fa_contig* d_contigs);

/* ---- K5: pafcov (replaces update_cov_vec, cigar.rs:710-741, and the per-thread array merge of
 *      pafcov.rs:29-53) ------------------------------------------------------------------------
 * Record i adds +1 to d_cov[cov_off[target_id[i]] + p] for every base p of its M / = ops that
 * lies below cov_len[target_id[i]].  Implemented as a difference array: accumulate() adds the
 * ±1 marks, finalize() turns marks into counts by an inclusive scan per target.  `total_cov` =
 * number of counters in d_cov (max over targets of cov_off + cov_len).  accumulate() may be
 * called for several batches before finalize(); it waits for its list pass twice (it reads two
 * counts back to size its work lists).  The context keeps its work lists between calls, grow-only:
 * 256 bytes per 1024 ops of the largest batch (the pieces as the list pass writes them) and 40 bytes
 * per piece (a record segment of a tile of ops under a window of 8192 counters; 3.5 per 1024 ops on
 * configs[3]'s records).  Context parameter "cov_spin_limit": polls of a neighbouring tile's sum
 * before a wave of the list pass adds up the ops itself (default 4096; 0: always adds them up).
 *
 * accumulate_final() = accumulate() of the LAST batch + finalize() in one pass over the array: the
 * kernel that replays the batch's marks window by window goes on to scan each window and hands its
 * sum to the windows behind it (decoupled look-back), so the array is read and written once instead
 * of twice more.  The targets' ranges [cov_off[t], cov_off[t] + cov_len[t]) must not overlap (any
 * order; WGA_E_INVALID_ARG otherwise — also from finalize()); counters between them are not touched.
 * The merge across the reference's per-thread arrays (pafcov.rs:29-53) has no counterpart: there is
 * one array. */
int wga_pafcov_accumulate(wga_ctx*, const wga_cigar_batch*, const uint32_t* d_target_id,
                          const uint64_t* d_t_start, const uint64_t* d_cov_off,
                          const uint64_t* d_cov_len, int32_t* d_cov, uint64_t total_cov);
int wga_pafcov_finalize(wga_ctx*, uint32_t n_targets, const uint64_t* d_cov_off,
                        const uint64_t* d_cov_len, int32_t* d_cov);
int wga_pafcov_accumulate_final(wga_ctx*, const wga_cigar_batch*, const uint32_t* d_target_id,
                                const uint64_t* d_t_start, const uint64_t* d_cov_off,
                                const uint64_t* d_cov_len, uint32_t n_targets, int32_t* d_cov,
                                uint64_t total_cov);

/* K18 — output bytes in HBM -> BGZF: what `-o out.maf.gz` stands for in the reference (utils.rs:181-228 wraps the output
 * file in flate2's GzEncoder, level 6, when the name ends in `.gz`; converter.rs / pafcov.rs / pseudomaf.rs write through
 * that writer).  The promise to a reader is a gzip stream that inflates to the plain output; this entry keeps it with the
 * text still on the device, so the compressed bytes are what crosses PCIe.  The stream is a sequence of complete gzip
 * members of at most 32 768 input bytes, each with the BGZF `BC` extra field (members are independent: seekable by
 * htslib-style readers, concatenable; any gzip reader takes the whole), each one deflate block of literals under the
 * member's own Huffman code, or a stored block where that is not smaller.  Calls on consecutive pieces of an output
 * concatenate into one valid stream; eof_marker != 0 appends BGZF's 28-byte empty member behind the last piece.
 *   wga_bgzf_bound(n)      what d_out must hold for n input bytes in the worst case (stored members + marker)
 *   wga_bgzf_compress(..)  d_in[n_bytes] -> d_out[*out_bytes]; synchronises once (the size); d_in, d_out any alignment.
 *                          d_out == NULL: the count call — *out_bytes is the exact size of the stream, nothing is written
 *                          (a caller that cannot spare wga_bgzf_bound's worst case allocates by it and calls again).
 *                          WGA_E_INVALID_ARG with *out_bytes set when out_cap is too small (nothing written). */
uint64_t wga_bgzf_bound(uint64_t n_bytes);
int wga_bgzf_compress(wga_ctx*, const uint8_t* d_in, uint64_t n_bytes, uint8_t* d_out, uint64_t out_cap, uint64_t* out_bytes,
                      int eof_marker);

/* pafcov's text back end (pafcov.rs:56-60): the BED lines
 * "<name>\t<pos>\t<pos+1>\t<count>\n" for positions p0 .. p0+count-1 of one target, d_cov pointing
 * at the counter of p0.  Two calls: with d_out == NULL it fills d_line_off[count+1] (exclusive
 * scan of the line lengths, total bytes in the last entry); the second call writes line k at
 * d_out + d_line_off[k]. */
int wga_pafcov_format(wga_ctx*, const uint8_t* d_name, uint32_t name_len, const int32_t* d_cov,
                      uint64_t p0, uint32_t count, uint64_t* d_line_off, uint8_t* d_out);

/* ---- per-record class sums of a batch: bases in M/=/X, I, D, S and "other" (N H P ...) ops.
 *      pafpseudo's host logic (pseudomaf.rs:147-202) needs M+X+D (target span) and the edited
 *      query length q_len - (I+S) + D before it can place segments.  d_sums: n x 5 u64.
 *      The call is the count call of pafpseudo's protocol: its tile and record sums stay in the
 *      context (88 bytes per 1024 ops + 40 per record, grow-only) for wga_pafpseudo_fill on the
 *      same batch arrays, which then does not compute them again (one-shot: that fill call consumes
 *      them; dropped when the op arrays are written through wga_memcpy_h2d / wga_memset or freed). --- */
typedef struct {
  uint64_t mx, i, d, s, o;
} wga_class_sums;
int wga_cigar_class_sums(wga_ctx*, const wga_cigar_batch*, wga_class_sums* d_sums);

/* ---- K6: pafpseudo row segments (replaces gen_pesudo_maf_by_cigar, cigar.rs:744-804, plus the
 *      overlap trim of pseudomaf.rs:190-192) ---------------------------------------------------
 * Record i writes its target-coordinate segment (length M+X+D, minus skip[i] leading columns)
 * at d_out + d_dst_off[i].  base_mode = 1: bases from q_fa (reverse-complemented for '-'),
 * 0: symbols '1' (M/=), '0' (X), '-' (D). */
int wga_pafpseudo_fill(wga_ctx*, const wga_cigar_batch*, int base_mode, const uint8_t* d_q_fa,
                       uint64_t q_fa_bytes, const uint64_t* d_q_src_off,
                       const uint64_t* d_q_src_len, const uint64_t* d_skip, uint8_t* d_out,
                       const uint64_t* d_dst_off, wga_rec_diag* d_diag);

/* ---- several devices in one process: the coverage reduce of a target whose records are spread over the devices
 *      (the element-wise merge of the reference's per-thread arrays, pafcov.rs:29-53, moved onto xGMI) ---------------------
 * ctxs[g] = a context on device g (ngpu distinct devices), d_bufs[g] = `count` int32 counters on that device.  After the
 * call, slice g of the index space — [count * g / ngpu, count * (g + 1) / ngpu) — of d_bufs[g] holds the element-wise sum
 * over all devices (a reduce-scatter); the rest of every buffer is unchanged.  Every device pulls its slice from every
 * other device (hipMemcpyPeer: all links busy at once, no ring) and adds it; the call synchronises all the contexts
 * before and after.  One host thread drives it (the contexts' owner threads must be idle). */
int wga_reduce_scatter_i32(wga_ctx** ctxs, int ngpu, int32_t** d_bufs, uint64_t count);

/* ---- utility: exclusive scan of n u64 values on device (d_out[n+1], d_out[n] = total) ------- */
int wga_exclusive_scan_u64(wga_ctx*, uint32_t n, const uint64_t* d_in, uint64_t* d_out);

/* ---- K20: MAF chunk (tools/chunk.rs:20-90 with recount_align_size parser/common.rs:179-190 and the record writer
 *      maf.rs:566-581) -----------------------------------------------------------------------------------------------------
 * A block's columns are those of its FIRST row (chunk.rs:35): chunks [0, L), [L, 2L), ... while a chunk ends before the block
 * does, then the rest; a block of 0 columns has one empty chunk.  Chunk k of a block is the record "a score=255\n", one line
 * "s\t<name>\t<start>\t<size>\t<+|->\t<srcSize>\t<text[c0 .. c1)>\n" per row and an empty line; size = the bytes of the slice
 * that are not '-', start = the row's input start plus the sizes of its chunks in front (plain addition on both strands).
 * Every row must hold at least c1 bytes of the chunks asked for (the reference panics on the slice; the caller cuts there).
 * A call writes a WINDOW: blocks d_blocks[0 .. n_blocks), each with the chunks [k_lo, k_hi) of it, in that order;
 * every entry has n_rows >= 1 and k_hi > k_lo, and a block (its rows) appears at most once in a window (its entries would
 * share d_carry: the later one's starts would be wrong).  n_lines = sum of n_rows * (k_hi - k_lo) < 2^32.  d_carry[row] = the sizes of the row's chunks written by earlier windows
 * (zero for a block's first window); the fill call adds this window's.  d_work = wga_maf_chunk_work_bytes(n_blocks,
 * n_lines) bytes of device memory the two calls share.  Two calls with the same arguments:
 *   d_out == NULL: the counts, starts and line lengths; *text_bytes = the window's text length (host value; synchronises).
 *   otherwise     : the text at d_out[0 .. text_bytes), and d_carry advanced. */
typedef struct {
  uint64_t seq_off;  /* the row's text: d_text[seq_off .. seq_off + seq_len) */
  uint64_t seq_len;
  uint64_t name_off; /* its name: d_text[name_off .. name_off + name_len) */
  uint64_t start;    /* the input start field */
  uint64_t src_size; /* the input srcSize field (the input size field is not used: the slices are counted) */
  uint32_t name_len;
  uint32_t strand_neg;
} wga_maf_chunk_row;
typedef struct {
  uint64_t row0;       /* the block's first row in the row table; its rows are row0 .. row0 + n_rows - 1 */
  uint64_t k_lo, k_hi; /* the block's chunks this window writes */
  uint32_t n_rows, pad;
} wga_maf_chunk_block;
uint64_t wga_maf_chunk_work_bytes(uint32_t n_blocks, uint64_t n_lines);
int wga_maf_chunk(wga_ctx*, const uint8_t* d_text, const wga_maf_chunk_row* d_rows, uint32_t n_blocks,
                  const wga_maf_chunk_block* d_blocks, uint64_t n_lines, uint64_t chunk_len, uint64_t* d_carry, void* d_work,
                  uint64_t* text_bytes, uint8_t* d_out);

/* ---- K21: MAF slices for maf-ext (tools/mafextra.rs:167-232 with MAFSLine::get_col_coord parser/maf.rs:81-95,
 *      MAFRecord::slice_block parser/maf.rs:223-248 and the record writer maf.rs:566-581) ----------------------------------
 * A HIT is one block cut by one region.  Its rows are d_rows[row0 .. row0 + n_rows), n_rows >= 1, in the block's order.
 *   whole != 0: the record as it was read: every row with its own start, size field and full text.
 *   otherwise : row `ord` is the ANCHOR (the row of the region's name) and [cut_lo, cut_hi), cut_lo <= cut_hi, are bases of
 *     the anchor counted from its start field (cut = region position - start).  col(p) = the index of the anchor's p-th
 *     (0-based) byte that is not '-', the anchor's length when it has p or fewer such bytes (maf.rs:81-95); so gap columns
 *     in front of base cut_lo are dropped and, once cut_hi reaches the anchor's non-gap count, every trailing gap column is
 *     kept.  With [c0, c1) = [col(cut_lo), col(cut_hi)) every row is written with text[c0 .. c1) and start = its start +
 *     cut_lo (plain addition whatever the row's strand and gaps: maf.rs:229, 239); size = cut_hi - cut_lo for the anchor
 *     (maf.rs:230) and the slice's bytes that are not '-' for every other row (maf.rs:241-243).
 * A record is "a score=255\n", one line "s\t<name>\t<start>\t<size>\t<+|->\t<srcSize>\t<text>\n" per row and an empty line.
 * A sliced hit with a row shorter than c1 is the reference's slice panic (maf.rs:233, 240): the call's text is that of the
 * hits in front of the first such hit, which *first_short_hit names (~0u: none).
 * The hits are written in their order; a block may appear in any number of hits; nothing is kept between calls.
 * Every hit's rows lie inside the table (row0 + n_rows <= n_table_rows, ord < n_rows) and n_hits <= 2^32 - 4: the caller's
 * contract, not checked.  n_lines = the sum of n_rows over the hits < 2^32; n_cols = the sum of seq_len over the n_table_rows table rows (every
 * table row gets a rank directory of one entry per 2048 columns: upload the rows that hits name).  d_work =
 * wga_maf_slice_work_bytes(...) bytes of device memory the two calls share.  Two calls with the same arguments:
 *   d_out == NULL: directories, cuts, sizes and line lengths; *text_bytes and *first_short_hit (host values; synchronises).
 *   otherwise     : the text at d_out[0 .. text_bytes). */
typedef struct {
  uint64_t seq_off;  /* the row's text: d_text[seq_off .. seq_off + seq_len) */
  uint64_t seq_len;
  uint64_t name_off; /* its name: d_text[name_off .. name_off + name_len) */
  uint64_t start;    /* the input start field */
  uint64_t size;     /* the input size field (written as it is by a whole hit) */
  uint64_t src_size; /* the input srcSize field */
  uint32_t name_len;
  uint32_t strand_neg;
} wga_maf_slice_row;
typedef struct {
  uint64_t row0;            /* the block's first row in the row table */
  uint64_t cut_lo, cut_hi;  /* the anchor's bases, relative to its start field */
  uint32_t n_rows, ord;     /* the block's rows; the anchor's index among them */
  uint32_t whole, pad;
} wga_maf_slice_hit;
uint64_t wga_maf_slice_work_bytes(uint32_t n_hits, uint64_t n_lines, uint64_t n_table_rows, uint64_t n_cols);
int wga_maf_slice(wga_ctx*, const uint8_t* d_text, const wga_maf_slice_row* d_rows, uint64_t n_table_rows, uint64_t n_cols,
                  uint32_t n_hits, const wga_maf_slice_hit* d_hits, uint64_t n_lines, void* d_work, uint64_t* text_bytes,
                  uint32_t* first_short_hit, uint8_t* d_out);

/* ---- K22: MAF block rewriter for filter and rename (tools/filter.rs:65-105, tools/rename.rs:7-23 with MAFRecord::rename
 *      parser/maf.rs:250-261 and the record writer maf.rs:566-581) ----------------------------------------------------------
 * A call works on a WINDOW: the blocks d_blocks[0 .. n_blocks) in that order, block b being the rows d_rows[row0 .. row0 +
 * n_rows) of the row table (K21's wga_maf_slice_row; every block's rows lie inside the table: the caller's contract).  Every
 * block that is KEPT is written as "a score=255\n", one line "s\t<prefix><name>\t<start>\t<size>\t<+|->\t<srcSize>\t<text>\n"
 * per row and an empty line: start, size and srcSize are the table's fields in decimal (the size is not recounted from the
 * text), the text is d_text[seq_off .. seq_off + seq_len).
 *   filter != 0: a block is dropped when its first row's size is below min_block_size or its second row's src_size is below
 *     min_query_size (filter.rs:96-101: both compare with `<`); a block with fewer than two rows is BAD (the reference indexes
 *     slines[1] before it compares: maf.rs:430).
 *   n_prefix != 0: row r's name is written behind prefix r, d_prefix_text[d_prefix_off[r] .. d_prefix_off[r + 1]) (an empty
 *     prefix is legal); a block whose n_rows differs from n_prefix is BAD (maf.rs:252-254).
 *   With neither set every block is kept as it is; a block of no rows is dropped.
 * The call's text is that of the kept blocks in front of the first bad block, which *first_bad_block names (~0u: none);
 * *n_kept counts them.  The selection is made on the device from the row table: the host does not look at a block again.
 * n_lines = the sum of n_rows over the window's blocks < 2^32.  d_work = wga_maf_rewrite_work_bytes(n_blocks, n_lines) bytes of
 * device memory the two calls share; d_out is 16-byte aligned.  Two calls with the same arguments, nothing else is kept:
 *   d_out == NULL: selection, places and line lengths; *text_bytes, *n_kept, *first_bad_block (host values; synchronises).
 *   otherwise     : the text at d_out[0 .. text_bytes); *text_bytes and *n_kept are read as the first call left them.
 * n_blocks == 0, or nothing kept: *text_bytes = 0 and success. */
typedef struct {
  uint64_t row0; /* the block's first row in the row table */
  uint32_t n_rows, pad;
} wga_maf_rewrite_block;
typedef struct {
  uint64_t min_block_size, min_query_size; /* used when filter != 0 */
  uint32_t filter;                         /* 0: keep every block (rename) */
  uint32_t n_prefix;                       /* 0: no prefixes (filter); else every block must have n_prefix rows */
  const uint8_t* d_prefix_text;            /* the prefixes' bytes */
  const uint32_t* d_prefix_off;            /* n_prefix + 1 offsets into d_prefix_text */
} wga_maf_rewrite_params;
uint64_t wga_maf_rewrite_work_bytes(uint32_t n_blocks, uint64_t n_lines);
int wga_maf_rewrite(wga_ctx*, const uint8_t* d_text, const wga_maf_slice_row* d_rows, uint32_t n_blocks,
                    const wga_maf_rewrite_block* d_blocks, uint64_t n_lines, const wga_maf_rewrite_params* params, void* d_work,
                    uint64_t* text_bytes, uint32_t* n_kept, uint32_t* first_bad_block, uint8_t* d_out);

/* ---- K24: `filter -f paf` — a line filter and the pair sums of `-a` (tools/filter.rs:88-160 with the csv writer of
 *      paf.rs:50-65) ----------------------------------------------------------------------------------------------------------
 * For a plain line (WGA_PAF_OK) the reference's writer reproduces the line's bytes whenever its nine numbers are in canonical
 * decimal: names and tags pass through as they are, only the numbers are printed anew.  Both entries work on d_text, n_bytes
 * and d_lines[n_lines] — the arguments and the result of wga_paf_split on the same text, with its limits: n_bytes < 0xFFFFFFF0,
 * 16 bytes of slack behind the text, n_lines < 2^32.  Both are called twice with the same arguments; the calls share d_work
 * (wga_paf_*_work_bytes(n_lines) bytes of device memory) and keep nothing else between them.  n_lines == 0: zero counts and
 * success.
 *
 * wga_paf_pairs looks only at WGA_PAF_OK lines; every other line gets d_pair_of_line[i] = 0xFFFFFFFF.  Two records are the same
 * PAIR exactly when their query-name bytes are equal and their target-name bytes are equal ("ab","c" and "a","bc" are two
 * pairs): a hash places a pair in the call's table, the names' bytes decide.  Pairs are numbered by ascending first_line, so
 * the numbering is the same for every call on the same lines.  A pair's sum is that of (num[5] - num[4]) over its records, the
 * difference and the sum wrapping mod 2^64 (filter.rs:118-127 in a release build).
 *   d_pairs == NULL and d_pair_of_line == NULL: the grouping; *n_pairs (host value; synchronises).
 *   otherwise: d_pair_of_line[n_lines] and d_pairs[*n_pairs] are written; cap_pairs >= *n_pairs (WGA_E_TOO_SMALL otherwise).
 * Context parameter "paf_pair_hash_bits" (1 .. 64, default 64): the hash is cut to that many low bits before it picks a place,
 * so that a test can make every pair collide.
 *
 * wga_paf_filter writes the text of the lines that are kept, in input order:
 *   selection  a WGA_PAF_SKIP line is never written.  A WGA_PAF_OK line is kept in threshold mode (d_pair_keep == NULL) unless
 *              (num[5] - num[4]) (wrapping) < min_block_size or num[0] < min_query_size (filter.rs:96-101: both compare with
 *              `<`), in pair mode when d_pair_keep[d_pair_of_line[i]] != 0 (filter.rs:143-152 with the caller's flags).
 *   text       a kept line's bytes from its first byte up to (not including) its `\n`, or up to n_bytes for an unterminated
 *              last line, and a `\n`.  *text_bytes = the sum of (length + 1) over the kept lines, *n_kept = their count.
 *   exactness  a line is INEXACT when it is WGA_PAF_FALLBACK, holds a byte >= 0x80, or is WGA_PAF_OK and one of its nine
 *              numbers (columns 2, 3, 4, 7 .. 12) starts with `+` or with `0` and another digit: the reference would write
 *              other bytes than the line's, or none.  Every line is checked, kept or not.  *first_inexact_line = the lowest
 *              such line, WGA_NONE when there is none.  If there is one, *text_bytes = 0, the second call writes nothing and
 *              the caller takes its csv-semantics path for this text.
 *   d_out == NULL: selection, line extents, places and the exactness check; the three host values (synchronises).
 *   otherwise     : the text at d_out[0 .. text_bytes); d_out is 16-byte aligned, no byte outside that extent is written;
 *                   *text_bytes and *n_kept are read as the first call left them. */
typedef struct {
  uint64_t first_line;           /* lowest line index of the pair */
  uint64_t sum;                  /* sum of (num[5] - num[4]) over the pair's records, both wrapping mod 2^64 */
  uint64_t qname_off, tname_off; /* the spans of first_line's names in d_text */
  uint32_t qname_len, tname_len;
} wga_paf_pair; /* 40 bytes */
uint64_t wga_paf_pairs_work_bytes(uint64_t n_lines);
int wga_paf_pairs(wga_ctx*, const uint8_t* d_text, uint64_t n_bytes, const wga_paf_line* d_lines, uint64_t n_lines, void* d_work,
                  uint64_t* n_pairs, uint32_t* d_pair_of_line, wga_paf_pair* d_pairs, uint64_t cap_pairs);
typedef struct {
  uint64_t min_block_size, min_query_size; /* used when d_pair_keep == NULL */
  const uint32_t* d_pair_of_line;          /* wga_paf_pairs' array for the same lines */
  const uint8_t* d_pair_keep;              /* one byte per pair; NULL: threshold mode */
} wga_paf_filter_params;
#define WGA_PAF_FILTER_TILE_BYTES 8192 /* the text leaves in tiles of this many bytes, one per block (tests place line ends by it) */
uint64_t wga_paf_filter_work_bytes(uint64_t n_lines);
int wga_paf_filter(wga_ctx*, const uint8_t* d_text, uint64_t n_bytes, const wga_paf_line* d_lines, uint64_t n_lines,
                   const wga_paf_filter_params*, void* d_work, uint64_t* text_bytes, uint64_t* n_kept,
                   uint64_t* first_inexact_line, uint8_t* d_out);

/* ---- K29: `validate --fix` — the plan and the end-fixing line writer (tools/validate.rs:71-141 with the csv writer of
 *      parser/paf.rs:50-65; replaces the record loop of the host's cmd_validate, which parsed every tag of every record into a
 *      string and printed every record again field by field) --------------------------------------------------------------
 * K24's observation applies unchanged: for a plain line whose nine numbers are in canonical decimal the csv writer gives back
 * the line's bytes, and `--fix` changes at most two of those numbers per record, column 4 (query_end) and column 9
 * (target_end).  Both entries work on d_text, n_bytes and d_lines[n_lines] — the arguments and the result of wga_paf_split on
 * the same text, with K24's limits: n_bytes < 0xFFFFFFF0, 16 bytes of slack behind the text, n_lines < 2^32.  Both are called
 * twice with the same arguments; the two calls of an entry share d_work (wga_paf_fix_work_bytes(n_lines) bytes of device
 * memory, 8-byte aligned) and keep nothing else between them; wga_paf_fix reads nothing wga_paf_fix_plan left there.
 * n_lines == 0: zero counts and success.
 *
 * wga_paf_fix_plan decides whether the text is TAKEN and where its CIGARs are.  A line is UNTAKEN when it is INEXACT by K24's
 * rule (WGA_PAF_FALLBACK, a byte >= 0x80, or WGA_PAF_OK with one of its nine numbers starting with `+` or with `0` and another
 * digit), or when it is WGA_PAF_OK with cg_beg == WGA_NONE (validate.rs:79 unwraps an error there: that text is the caller's
 * csv-semantics path's).  Every line is checked.
 *   d_cg_beg == NULL and d_cg_end == NULL: *n_records = the number of WGA_PAF_OK lines, *first_untaken_line = the lowest
 *              untaken line, WGA_NONE when the text is taken (host values; synchronises).  If a line is untaken,
 *              *n_records = 0.
 *   otherwise: d_cg_beg[*n_records] and d_cg_end[*n_records], the records' cg:Z: spans in line order (wga_cigar_tokenise_spans'
 *              arguments); no other byte is written, and nothing at all when *n_records == 0.
 *
 * wga_paf_fix writes three texts from d_counts[n_records], wga_cigar_stat's counts of the records in line order (n_records =
 * the number of WGA_PAF_OK lines, WGA_E_INVALID_ARG otherwise).  For record k on line i, wrapping mod 2^64 as the release build:
 *   eq = num[1] + match + mismatch + ins_bp + inv_ins_bp,  et = num[4] + match + mismatch + del_bp + inv_del_bp
 *   rows   for every WGA_PAF_OK line, in input order: the line's bytes from its first byte up to (not including) its `\n`, or
 *          up to n_bytes for an unterminated last line, with column 4 replaced by the canonical decimal of eq when
 *          eq != num[2] and column 9 by that of et when et != num[5], then `\n`.  WGA_PAF_SKIP lines are not written.  The
 *          columns are found by their tabs from the line's first byte (a taken line has no tab inside a name).
 *   qlist  for every record with eq != num[2], in input order: `<qname>:<num[1]>-<num[2]>\n` (the old end).
 *   tlist  likewise `<tname>:<num[4]>-<num[5]>\n` for et != num[5].
 *   d_rows == d_qlist == d_tlist == NULL: places and sizes; *sizes (host values; synchronises).
 *   otherwise: every text whose pointer is not NULL at [0, *_bytes) of its buffer (16-byte aligned), no byte outside that
 *              extent; *sizes is read as the first call left it.
 * The call is meant for a text wga_paf_fix_plan takes; on any other it reads and writes nothing outside its arguments'
 * extents, and its texts are not specified. */
typedef struct {
  uint64_t rows_bytes, qlist_bytes, tlist_bytes;
  uint64_t n_records, n_q_bad, n_t_bad;
} wga_paf_fix_sizes; /* 48 bytes */
#define WGA_PAF_FIX_TILE_BYTES 8192 /* the rows leave in tiles of this many bytes, one per block (tests place edits by it) */
uint64_t wga_paf_fix_work_bytes(uint64_t n_lines);
int wga_paf_fix_plan(wga_ctx*, const uint8_t* d_text, uint64_t n_bytes, const wga_paf_line* d_lines, uint64_t n_lines, void* d_work,
                     uint64_t* n_records, uint64_t* first_untaken_line, uint64_t* d_cg_beg, uint64_t* d_cg_end);
int wga_paf_fix(wga_ctx*, const uint8_t* d_text, uint64_t n_bytes, const wga_paf_line* d_lines, uint64_t n_lines,
                const wga_cigar_counts* d_counts, uint64_t n_records, void* d_work, wga_paf_fix_sizes* sizes, uint8_t* d_rows,
                uint8_t* d_qlist, uint8_t* d_tlist);

/* ---- K25: `filter -f chain` — the chain record writer (replaces the formatting loop of the host's cmd_filter_chain,
 *      wgatools_amd/host/cmd_filter.inc:345-382 of the commit before it: every data line downloaded as 24 bytes and printed by
 *      one CPU thread; in the reference chain.rs:92-100,185-204 behind the selection of tools/filter.rs:17-39,91-105) ---------
 * d_text, d_heads[n_chains], d_lines and d_line_off[n_chains + 1] are wga_chain_split's arguments and results for a file it
 * took (WGA_CHAIN_OK), or arrays of the same meaning: d_line_off[0] = 0, d_line_off ascending, d_line_off[n_chains] = the
 * number of data lines (the call reads it from there), the names' spans inside d_text.  For every KEPT chain r, in input order:
 *   chain\t<score>\t<tname>\t<tsize>\t<+|->\t<tstart>\t<tend>\t<qname>\t<qsize>\t<+|->\t<qstart>\t<qend>\t<id>
 *   then per data line   \n<size>\t<col2>\t<col3>
 *   then                 \n\n
 * All numbers in canonical decimal (the score is num[0]: 1 to 15 digits for a file the splitter takes, whose f64 Display is that
 * decimal), the names copied from d_text.  Chain r is DROPPED when (num[3] - num[2]) (wrapping) < min_block_size or num[4] <
 * min_query_size (filter.rs:96-101: both compare with `<`).  A chain with d_line_off[r] == d_line_off[r + 1] is legal here: its
 * text is the header and "\n\n".
 *   d_out == NULL: the selection, the byte count of every header and data line and their places; *total_bytes and *n_kept
 *                  (host values: the call reads d_line_off[n_chains], then both totals in one copy).
 *   otherwise    : the text at d_out[0 .. *total_bytes); d_out may have any alignment, the caller leaves 16 bytes of slack
 *                  behind it; no byte in front of d_out and none from d_out + *total_bytes + 16 on is touched (this
 *                  implementation writes none outside the text).  *total_bytes and *n_kept are read as the first call left
 *                  them; the selection and the places are the first call's (d_work), so the two calls take the same arguments.
 * n_chains == 0: zero counts, nothing written.  WGA_E_INVALID_ARG: n_chains + data lines > 0xFFFFFFF0, a null array with
 * n_chains > 0, a null d_work.
 * d_work: wga_chain_filter_work_bytes(n_chains, n_data_lines) bytes of device memory, 8-byte aligned, shared by the two calls
 * = 8 * (n_chains + N + 2 + N / 1024 + 4) with N = n_chains + n_data_lines: 8 bytes per chain (the plan) and 8 per chain and
 * data line (the scan of the item sizes), plus the scan's partial sums. */
typedef struct {
  uint64_t min_block_size, min_query_size;
} wga_chain_filter_params; /* 16 bytes */
uint64_t wga_chain_filter_work_bytes(uint64_t n_chains, uint64_t n_data_lines);
int wga_chain_filter(wga_ctx*, const uint8_t* d_text, uint64_t n_bytes, const wga_chain_head* d_heads, uint64_t n_chains,
                     const uint64_t* d_lines, const uint64_t* d_line_off, const wga_chain_filter_params*, void* d_work,
                     uint64_t* total_bytes, uint64_t* n_kept, uint8_t* d_out);

/* ---- K26: `dotplot --out-format csv`, base-level — the csv row writer (replaces the row loop of the host's dotplot_rows,
 *      wgatools_amd/host/cmd_dotplot.inc:41-58 of the commit before it: every segment downloaded as 40 bytes and printed by one
 *      CPU thread; in the reference the csv writer of tools/dotplot.rs:208-262 over emit_baseplotdatas, cigar.rs:815-914) -----
 * d_segs (5 u64 per segment: four numbers and the kind 0 M / 1 I / 2 D) and d_seg_off[n + 1] are wga_cigar_dotplot's result and
 * the scan of its counts, or arrays of the same meaning: d_seg_off[0] = 0, d_seg_off ascending, equal neighbours = a record
 * without segments, d_seg_off[n] = the number of rows N (the call reads it from there).  d_tails[d_tail_off[i] ..
 * d_tail_off[i + 1]) is record i's TAIL, the bytes `,<ref_chro>,<query_chro>\n` as the caller's csv quoting made them: opaque
 * bytes of any length >= 1, copied as they are.  For every segment, in order:
 *   <s0>,<s1>,<s2>,<s3>,<M|I|D>   then its record's tail
 * The numbers in canonical decimal.  A kind above 2 is the caller's error: its letter is `?`, nothing is indexed by it.
 *   d_out == NULL: the byte count of every row and the rows' places (d_work); *total_bytes (a host value: the call reads
 *                  d_seg_off[n], then the total).
 *   otherwise    : the text at d_out[0 .. *total_bytes) with the places of the first call; d_out may have any alignment, the
 *                  caller leaves 16 bytes of slack behind it; no byte in front of d_out and none from d_out + *total_bytes + 16
 *                  on is touched (this implementation writes none outside the text).  *total_bytes is read as the first call
 *                  left it, so the two calls take the same arguments.
 * n == 0 or N == 0: total 0, nothing written.  WGA_E_INVALID_ARG: N > 0xFFFFFFF0 (refused before a segment is read), a null
 * array with n > 0, a null d_work with N > 0.
 * d_work: wga_dotplot_csv_work_bytes(N) bytes of device memory, 8-byte aligned, shared by the two calls
 * = 8 * (N + 1 + N / 1024 + 4): 8 bytes per row (its size, then its place) plus the scan's partial sums. */
uint64_t wga_dotplot_csv_work_bytes(uint64_t n_rows);
int wga_dotplot_csv(wga_ctx*, uint32_t n, const uint64_t* d_segs, const uint64_t* d_seg_off, const uint8_t* d_tails,
                    const uint64_t* d_tail_off, void* d_work, uint64_t* total_bytes, uint8_t* d_out);

/* ---- K27: `chain2paf` — the PAF record writer (replaces the record loop of the host's chain2paf_range,
 *      wgatools_amd/host/cmd_chain.inc: every head downloaded, the lines turned into packed ops for K1's two sums, twelve columns
 *      per record printed by one CPU thread and scattered around the CIGAR text; in the reference convert2paf chain.rs:430-452
 *      over parse_chain_to_cigar cigar.rs:554-627, written by the csv writer of converter.rs:391-416) ----------------------------
 * d_text, d_heads[n_chains], d_lines and d_line_off[n_chains + 1] are wga_chain_split's arguments and results for a file it
 * took (WGA_CHAIN_OK), or arrays of the same meaning: d_line_off[0] = 0, d_line_off ascending, d_line_off[n_chains] = the
 * number of data lines (the call reads it from there), the names' spans inside d_text[0 .. n_bytes).  For every chain r, in
 * input order, one record:
 *   <qname>\t<qsize>\t<qstart>\t<qend>\t<+|->\t<tname>\t<tsize>\t<tstart>\t<tend>\t<matches>\t<block_length>\t255\tcg:Z:
 *   then per data line   <size>M   <col3>I when col3 != 0   <col2>D when col2 != 0      ("0M" for a size of 0)
 *   then                 \n
 * The numbers are num[4], num[5], num[6] and num[1], num[2], num[3] unchanged, in canonical decimal; the strand is the query's
 * (the target's is not printed).  matches = the sum of the chain's sizes, block_length = matches + the sum of its 2nd columns,
 * both mod 2^64 (mismatch is 0; a deletion counts once whichever strand books it).  A name is written as the csv writer with a
 * tab delimiter and QuoteStyle::Necessary writes it: as it is, unless it holds a tab, a quote, CR or LF (a name the splitter
 * takes can only hold the quote); then between quotes with every quote inside doubled.  A chain with d_line_off[r] ==
 * d_line_off[r + 1] is legal here: its record ends in "cg:Z:\n".
 *   d_out == NULL: the sums, the byte count of every head and data line and their places (d_work); *total_bytes (a host value:
 *                  the call reads d_line_off[n_chains], then the total).
 *   otherwise    : the text at d_out[0 .. *total_bytes) with the sums and places of the first call; d_out may have any
 *                  alignment, the caller leaves 16 bytes of slack behind it; no byte in front of d_out and none from d_out +
 *                  *total_bytes + 16 on is touched (this implementation writes none outside the text).  *total_bytes is read as
 *                  the first call left it, so the two calls take the same arguments.
 * n_chains == 0: total 0, nothing written.  WGA_E_INVALID_ARG: n_chains + data lines > 0xFFFFFFF0 (refused before anything is
 * read beyond d_line_off[n_chains]), a null array with n_chains > 0, a null d_work.
 * d_work: wga_chain2paf_work_bytes(n_chains, n_data_lines) bytes of device memory, 8-byte aligned, shared by the two calls
 * = 8 * (3 C + N + 1 + 2 (L + 1) + N / 1024 + 4) with C = n_chains, L = n_data_lines, N = C + L: 24 bytes per chain (the head's
 * byte count and the two sums), 8 per chain and data line (the scan of the item sizes), 16 per data line (the wrapping scans of
 * the sizes and of the 2nd columns), plus the scans' partial sums. */
uint64_t wga_chain2paf_work_bytes(uint64_t n_chains, uint64_t n_data_lines);
int wga_chain2paf(wga_ctx*, const uint8_t* d_text, uint64_t n_bytes, const wga_chain_head* d_heads, uint64_t n_chains,
                  const uint64_t* d_lines, const uint64_t* d_line_off, void* d_work, uint64_t* total_bytes, uint8_t* d_out);

/* ---- K28: `maf2paf` — the PAF record writer (replaces the record loop of the host's maf2paf_rows,
 *      wgatools_amd/host/cmd_maf2paf.inc of the commit before it: the run offsets, the text sizes and the counters of every block
 *      downloaded, twelve columns and NM:i: per record printed by host threads and scattered around the CIGAR text; in the
 *      reference the record of maf.rs:484-520, written by the csv writer of converter.rs:29-54) --------------------------------
 * d_counts[n] and d_runs, d_run_off[n + 1], d_cols[n] are wga_maf_pair_stat's results and arguments for n blocks, or arrays of
 * the same meaning: d_run_off[0] = 0, d_run_off ascending, d_run_off[n] = the number of runs (the call reads it from there), a
 * run = start column << 3 | class.  d_heads[n] holds the numbers the caller prints and the spans of the two names inside
 * d_names[0 .. n_name_bytes).  For every block r, in input order, one record:
 *   <qname>\t<q0>\t<q1>\t<q2>\t<+|->\t<tname>\t<t0>\t<t1>\t<t2>\t<matches>\t<block_length>\t255\tNM:i:<block_length - matches>\tcg:Z:
 *   then per run   <length><=|I|D|X>
 *   then           \n
 * The numbers are q[0 .. 2] and t[0 .. 2] unchanged, in canonical decimal.  matches = d_counts[r].match, block_length = match +
 * mismatch + ins_bp + inv_ins_bp + del_bp + inv_del_bp of d_counts[r], NM = block_length - matches, all mod 2^64.  A run's
 * length is the next run's start (d_cols[r] for the block's last run) minus its own; its letter is its class, the low 3 bits:
 * 0 `=`, 1 `I`, 2 `D`, anything else `X` — byte for byte what wga_maf_runs_cigar_text prints for the same arrays.  A name is
 * written as the csv writer with a tab delimiter and QuoteStyle::Necessary writes it: as it is, unless it holds a tab, a
 * quote, CR or LF; then between quotes with every quote inside doubled.  A name whose span does not lie inside d_names is
 * written as empty.  A block with d_run_off[r] == d_run_off[r + 1] is legal here: its record ends in "cg:Z:\n".
 *   d_out == NULL: the sums, the byte count of every head and run and their places (d_work); *total_bytes (a host value: the
 *                  call reads d_run_off[n], then the total).
 *   otherwise    : the text at d_out[0 .. *total_bytes) with the sums and places of the first call; d_out may have any
 *                  alignment, the caller leaves 16 bytes of slack behind it; no byte in front of d_out and none from d_out +
 *                  *total_bytes + 16 on is touched (this implementation writes none outside the text).  *total_bytes is read as
 *                  the first call left it, so the two calls take the same arguments.
 * n == 0: total 0, nothing written.  WGA_E_INVALID_ARG: n + runs > 0xFFFFFFF0 (refused before anything is read beyond
 * d_run_off[n]), a null array with n > 0 (d_names only when n_name_bytes > 0, d_runs only when there are runs), a null d_work.
 * d_work: wga_maf2paf_work_bytes(n, n_runs) bytes of device memory, 8-byte aligned, shared by the two calls
 * = 8 * (3 n + N + 1 + N / 1024 + 4) with N = n + n_runs: 24 bytes per block (the head's byte count and the two sums), 8 per
 * block and run (the scan of the item sizes), plus the scan's partial sums. */
typedef struct {
  uint64_t q[3];                 /* query_length, query_start, query_end as printed */
  uint64_t t[3];                 /* target_length, target_start, target_end as printed */
  uint64_t qname_off, tname_off; /* spans of d_names */
  uint32_t qname_len, tname_len;
  uint8_t strand_neg, pad[7];
} wga_maf2paf_head; /* 80 bytes */
uint64_t wga_maf2paf_work_bytes(uint64_t n, uint64_t n_runs);
int wga_maf2paf(wga_ctx*, uint32_t n, const uint8_t* d_names, uint64_t n_name_bytes, const wga_maf2paf_head* d_heads,
                const wga_cigar_counts* d_counts, const uint64_t* d_runs, const uint64_t* d_run_off, const uint64_t* d_cols,
                void* d_work, uint64_t* total_bytes, uint8_t* d_out);

/* ---- K30: `paf2chain`, `maf2chain` — the chain heads (replaces the record loop of the host's paf2chain_range and maf2chain_text,
 *      wgatools_amd/host/cmd_chain.inc: the trims, text sizes and diagnostics of every record downloaded, the head printed by one
 *      CPU thread, the heads and two offset arrays uploaded and scattered around the data lines; in the reference ChainHeader's
 *      Display chain.rs:185-203 behind the TryFrom arithmetic of chain.rs:103-183) ------------------------------------------------
 * d_trim[n], d_nbytes[n] and d_diag[n] are the results of wga_cigar_chain's count call for n records, or arrays of the same
 * meaning.  d_heads[n] reuses wga_maf2paf_head: q[0 .. 2] / t[0 .. 2] = size, start and end BEFORE trimming, the spans of the two
 * names inside d_names[0 .. n_name_bytes), strand_neg = the query's strand.  n_good = the smallest r with
 * d_diag[r].bad_op_idx != WGA_NONE, or n.  For every record r < n_good, in input order:
 *   chain\t255\t<tname>\t<t[0]>\t+\t<ts>\t<te>\t<qname>\t<q[0]>\t<+|->\t<qs>\t<qe>\t<chain_id0 + r>
 *   then  d_nbytes[r] bytes that this call does NOT write: wga_cigar_chain's text of the record, at d_data_off[r]
 *   then  \n\n
 * with, all mod 2^64 and in canonical decimal,
 *   ts = t[1] + head_del, te = t[2] - tail_del
 *   `+`: qs = q[1] + head_ins,          qe = q[2] - tail_ins
 *   `-`: qs = q[0] - (q[2] - head_ins), qe = q[0] - (qs + tail_ins) with the qs just computed (chain.rs:136-137,177-178).
 * A name is written as it is (`write!`, no quoting); a name whose span does not lie inside d_names is written as empty.
 *   d_out == NULL: the byte count of every head and the place of every record (d_work), d_data_off[n] (device memory:
 *                  d_data_off[r] = the place of record r's data lines behind its head; from n_good on the text's length);
 *                  *total_bytes and *n_good (host values; the call synchronises).
 *   otherwise    : the heads and the "\n\n" of records [0, n_good) with the places of the first call, and not one byte else:
 *                  the d_nbytes[r] bytes at d_data_off[r] are wga_cigar_chain's (its fill call with d_data_off and n = n_good,
 *                  on the same stream in either order).  d_out may have any alignment, the caller leaves 16 bytes of slack behind
 *                  the text; no byte in front of d_out and none from d_out + *total_bytes + 16 on is touched (this
 *                  implementation writes none outside the heads and record ends).  *total_bytes and *n_good are read as the
 *                  first call left them, so the two calls take the same arguments.
 * n == 0, or a fill with a total of 0: nothing is written.  WGA_E_INVALID_ARG: a null d_work, total_bytes or n_good, a null array
 * with n > 0 (d_names only when n_name_bytes > 0).
 * d_work: wga_chain_heads_work_bytes(n) bytes of device memory, 8-byte aligned, shared by the two calls
 * = 8 * (2 n + 2 + n / 1024 + 4): 8 bytes per record for the plan (its head's byte count), 8 per record and one more for the
 * scan (its place; the total last), one word for n_good (the min-reduction over d_diag), plus the scan's partial sums. */
uint64_t wga_chain_heads_work_bytes(uint64_t n);
int wga_chain_heads(wga_ctx*, uint32_t n, const uint8_t* d_names, uint64_t n_name_bytes, const wga_maf2paf_head* d_heads,
                    const wga_chain_trim_t* d_trim, const uint64_t* d_nbytes, const wga_rec_diag* d_diag,
                    uint64_t chain_id0, void* d_work, uint64_t* d_data_off, uint64_t* total_bytes, uint32_t* n_good,
                    uint8_t* d_out);

/* ---- K31: `pafpseudo` — the row frame writer (replaces the row strings of the host's cmd_pafpseudo, wgatools_amd/host/
 *      cmd_pafpseudo.inc: `text.append(gap, '-')`, one append per segment, `append(tail, '-')`, the target row as `append(size, 'N')`
 *      or a slice of the pool, the `s` line heads and line ends; in the reference pseudomaf.rs:98-209) ---------------------------
 * A file's text, or a run of whole lines of it, is described by n_items spans, and this call writes every byte of it that is not a
 * segment: wga_pafpseudo_fill (K6) writes those, with d_dst_off pointing at their places in the same buffer.
 * Item layout.  The items tile d_out[0, out_bytes) in order without gaps: item[0].dst == 0, item[k + 1].dst == item[k].dst +
 *   item[k].len, and the last item ends at out_bytes.  Items without bytes are allowed, and runs of them.  d_out must be 16-byte
 *   aligned (wga_malloc gives 256), else WGA_E_INVALID_ARG.  All offsets and lengths are 64-bit.
 * Bad items.  *d_first_bad (device memory) receives WGA_NONE, or the index of the first item that breaks the tiling (its dst is
 *   not the end of the item in front, it does not lie inside [0, out_bytes), it is the last and does not end at out_bytes), has a
 *   kind above WGA_SPAN_HOLE, or names a copy range that does not lie inside its source.  A bad item writes nothing, and neither
 *   do the items behind the first bad one (where they belong is not defined); the items in front of it are written.  No byte
 *   outside d_out[0, out_bytes) is written, whatever the items say.
 * Bytes written.  Every byte of a FILL or COPY item is written exactly once.  Every byte of a HOLE and every byte outside
 *   [0, out_bytes) is left as it was — the ragged ends of 16-byte groups included: a group that a hole or the end of the text
 *   shares with other items is written in narrower stores.  K6's fill and this call may therefore run in either order on the
 *   stream, and each output byte is written once.
 * Source reads stay inside d_pool[0, pool_bytes) and d_text[0, text_bytes): a source's ends are read without reaching over them
 *   (the CLI's pool has 32 bytes of padding at both ends; this call does not ask for it).  Either source may be null when its
 *   size is 0.
 * n_items == 0 is valid with out_bytes == 0 only (nothing is written, *d_first_bad = WGA_NONE).  WGA_E_INVALID_ARG: a null
 * d_first_bad, null d_items or d_out with n_items > 0, a null source of a size above 0, a misaligned d_out, n_items == 0 with
 * out_bytes > 0, out_bytes of 2^47 or more.
 * The work is dealt out in tiles of WGA_PSEUDO_FRAME_TILE output bytes, whatever the items' lengths. */
#define WGA_SPAN_FILL      0u  /* len copies of the byte in the low 8 bits of src                 */
#define WGA_SPAN_COPY_POOL 1u  /* d_pool[src .. src+len)                                          */
#define WGA_SPAN_COPY_TEXT 2u  /* d_text[src .. src+len)  (heads, "a score=0\n", newlines)        */
#define WGA_SPAN_HOLE      3u  /* bytes another kernel writes (K6's segments): left untouched     */
typedef struct { uint64_t dst, len, src; uint32_t kind, pad; } wga_span_item;   /* 32 bytes */
#define WGA_PSEUDO_FRAME_TILE 65536u /* output bytes per block */

int wga_pafpseudo_frame(wga_ctx*, uint64_t n_items, const wga_span_item* d_items,
                        const uint8_t* d_pool, uint64_t pool_bytes,
                        const uint8_t* d_text, uint64_t text_bytes,
                        uint8_t* d_out, uint64_t out_bytes, uint64_t* d_first_bad);

/* ---- K32: `paf2maf`, `chain2maf` — the MAF record frames (replaces ExpandJob::add and the frame part of expand_batch,
 *      wgatools_amd/host/wgatools_main.cpp: three strings per record built by one CPU thread, the counts and three offset arrays
 *      downloaded, 3 n destinations computed, the blob, its offsets and the destinations uploaded and scattered, every diagnostic
 *      downloaded; in the reference MAFWriter::write_record maf.rs:566-581 behind converter.rs:196-263 and :288-355) ---------------
 * d_counts[n] are wga_cigar_stat's counters and d_t_src_len[n] / d_q_src_len[n] the lengths of the fetched slices, as for
 * wga_paf2maf_layout; d_heads[n] the numbers AS PRINTED and the spans of the two names inside d_names[0 .. n_name_bytes).  Record
 * r, in input order, is
 *   a score=<score>\n
 *   s\t<tname>\t<t[0]>\t<t[1]>\t<+|->\t<t[2]>\t          the target head
 *   then  d_t_src_len[r] + ins_bp + inv_ins_bp bytes that this call does NOT write: the target row, at d_t_row_off[r]
 *   \ns\t<qname>\t<q[0]>\t<q[1]>\t<+|->\t<q[2]>\t        the query head
 *   then  d_q_src_len[r] + del_bp + inv_del_bp bytes that this call does NOT write: the query row, at d_q_row_off[r]
 *   \n\n
 * with every number in canonical decimal of its 64-bit value.  A name is written as it is (`format!`, no quoting); a name whose
 * span does not lie inside d_names is written as empty.
 *   d_out == NULL: the byte counts of every record's two heads (d_work); d_t_row_off[n], d_q_row_off[n] and d_rec_off[n + 1]
 *                  (device memory; d_rec_off[n] = the text's length): exactly what wga_paf2maf_layout gives for pre_t / pre_q =
 *                  those head lengths and post = 2, so wga_paf2maf_expand takes them unchanged; *total_bytes (a host value; the
 *                  call synchronises).  d_diag is not read; *n_good = n and *good_bytes = *total_bytes.
 *   otherwise    : every frame byte of all n records at the places of the first call, and not one byte else: the rows' bytes are
 *                  left as they were, the ragged ends of 16-byte groups that a frame shares with a row included (narrower stores
 *                  there), so wga_paf2maf_expand may run before or after this call on the stream.  *n_good = the smallest r
 *                  whose d_diag[r] has bad_op_idx, panic_op_idx or bad_base_pos set, n when there is none or d_diag is NULL;
 *                  *good_bytes = d_rec_off[*n_good] (host values; the call synchronises).  The frames behind n_good are written
 *                  as well: the caller cuts the text at *good_bytes.  d_out may have any alignment, the caller leaves 16 bytes
 *                  of slack behind the text; no byte in front of d_out and none from d_out + *total_bytes on is written.
 *                  *total_bytes is read as the first call left it, so the two calls take the same arguments.
 * All places are 64-bit: a text beyond 4 GiB is the normal case of a resident batch.
 * n == 0: *total_bytes = 0, *n_good = 0, nothing is written.  WGA_E_INVALID_ARG: a null d_work, total_bytes, n_good or good_bytes,
 * whatever n; a null array with n > 0 (d_names only when n_name_bytes > 0; d_diag may always be null).
 * d_work: wga_paf2maf_frame_work_bytes(n) bytes of device memory, 8-byte aligned, shared by the two calls
 * = 8 * (2 n + 2 + n / 1024 + 4): 8 bytes per record for each of the two heads' byte counts, one word for n_good (the
 * min-reduction over d_diag) and one for good_bytes, plus the scan's partial sums. */
typedef struct {
  uint64_t score;                 /* as printed */
  uint64_t t[3], q[3];            /* start, aligned size, source size — as printed (the caller has already
                                     turned a '-' query's start into q_size - q_end, mod 2^64) */
  uint64_t tname_off, qname_off;  /* spans of d_names */
  uint32_t tname_len, qname_len;
  uint8_t  t_neg, q_neg, pad[6];
} wga_maf_frame_head;             /* 88 bytes */

uint64_t wga_paf2maf_frame_work_bytes(uint64_t n);
int wga_paf2maf_frame(wga_ctx*, uint32_t n, const uint8_t* d_names, uint64_t n_name_bytes,
                      const wga_maf_frame_head* d_heads, const wga_cigar_counts* d_counts,
                      const uint64_t* d_t_src_len, const uint64_t* d_q_src_len,
                      const wga_rec_diag* d_diag, void* d_work,
                      uint64_t* d_t_row_off, uint64_t* d_q_row_off, uint64_t* d_rec_off,
                      uint64_t* total_bytes, uint32_t* n_good, uint64_t* good_bytes, uint8_t* d_out);

/* ---- K33: `stat --each` — the TSV rows (replaces, for `-e`, the per-record StatInput / Statistic structs, the stable_sort over
 *      all of them and the row printing of stat_tsv, wgatools_amd/host/wga_host.cpp: 17 integers, 2 names and 3 floats per row from
 *      one CPU thread; in the reference split_final stat.rs:129-164 through the csv writer of stat.rs:117-123, over the
 *      per-record statistics of common.rs:116-140) ---------------------------------------------------------------------------
 * d_counts[n] are wga_cigar_stat's or wga_maf_pair_stat's counters; d_heads[n] the four numbers AS PRINTED and the spans of the
 * two names inside d_names[0 .. n_name_bytes).  Row r, in input order, is ONE line of 22 columns, tabs between them:
 *   <ref_name> <ref_size> <ref_start> <query_name> <query_size> <query_start> <aligned_size> 0 <identity> <similarity>
 *   <matched> <mismatched> <ins_event> <del_event> <ins_size> <del_size> <inv_event> <inv_size>
 *   <inv_ins_event> <inv_ins_size> <inv_del_event> <inv_del_size> \n
 * with c = d_counts[r] and all integer arithmetic mod 2^64:
 *   aligned_size = match + mismatch + del_bp + inv_del_bp            (unaligned_size is the literal 0 in this mode)
 *   identity     = (float)match / (float)aligned_size
 *   similarity   = (float)(match + mismatch) / (float)aligned_size
 *   inv_size     = inv_ev != 0 ? (float)(aligned_size + match + mismatch + ins_bp + inv_ins_bp) / (float)(inv_ev + 1) : 0.0f
 * u64 -> f32 rounds to nearest even and the division is the IEEE single precision one.  Integers are printed in canonical
 * decimal.  A name is written as the csv writer does under QuoteStyle::Necessary with a tab delimiter (as it is, unless it holds
 * a tab, a quote, CR or LF: then between quotes, every quote inside doubled); a name whose span does not lie inside d_names is
 * written as empty.  An f32 is written as ryu does (wga_f32_text below).
 *   d_out == NULL: the byte count of every row (d_work), d_row_off[n + 1] (device memory; d_row_off[n] = the text's length)
 *                  and *total_bytes (a host value; the call synchronises).
 *   otherwise    : the text at d_out[0 .. *total_bytes).  d_out may have any alignment, the caller leaves 16 bytes of slack
 *                  behind the text; no byte in front of d_out and none from d_out + *total_bytes on is written.  *total_bytes,
 *                  d_work and d_row_off are read as the first call left them, so the two calls take the same arguments.  A row
 *                  whose span in d_row_off is not its byte count in d_work is not written.
 * All places are 64-bit.  n == 0: *total_bytes = 0, nothing is written.  WGA_E_INVALID_ARG: a null d_work or total_bytes,
 * whatever n; a null array with n > 0 (d_names only when n_name_bytes > 0); n > 0xFFFFFFF0.
 * d_work: wga_stat_rows_work_bytes(n) bytes of device memory, 8-byte aligned, shared by the two calls
 * = 8 * (n + n / 1024 + 4): 8 bytes per row for its byte count, plus the scan's partial sums (32 bytes for n == 0). */
typedef struct {
  uint64_t ref_size, ref_start, query_size, query_start;   /* as printed */
  uint64_t rname_off, qname_off;                            /* spans of d_names */
  uint32_t rname_len, qname_len;
} wga_stat_row_head;                                        /* 56 bytes */

uint64_t wga_stat_rows_work_bytes(uint64_t n);
int wga_stat_rows(wga_ctx*, uint32_t n, const uint8_t* d_names, uint64_t n_name_bytes,
                  const wga_stat_row_head* d_heads, const wga_cigar_counts* d_counts,
                  void* d_work, uint64_t* d_row_off /* n + 1, device */, uint64_t* total_bytes, uint8_t* d_out);

/* the formatter alone, for tests: d_text[16 i ..] receives the text of the f32 with bit pattern d_bits[i], d_len[i] its length
 * (at most 16; the bytes of d_text behind a text are left as they were).  NaN -> "NaN", +-inf -> "inf" / "-inf", +-0 -> "0.0" /
 * "-0.0", anything else the shortest digits that read back as the same f32, the closest such to the value, laid out as
 * ryu::Buffer::format does: with the digits' count len, the decimal exponent k of the last digit and kk = len + k
 *   0 <= k && kk <= 13 : digits, k zeros, ".0"         0 < kk <= 13 : dddd.ddd
 *   -6 < kk <= 0       : "0.", -kk zeros, digits       else         : d[.ddd]e<kk - 1>
 * n == 0 is valid; WGA_E_INVALID_ARG: a null array with n > 0, n > 0xFFFFFFF0. */
int wga_f32_text(wga_ctx*, uint64_t n, const uint32_t* d_bits, uint8_t* d_text, uint8_t* d_len);

/* ---- K34: `dotplot -m overview` — the csv rows (replaces the per-record loop of dotplot_rows, wgatools_amd/host/cmd_dotplot.inc:
 *      the counters downloaded, then four integers, one f64 and two quoted names per row from one CPU thread; in the reference
 *      rec_dot_data tools/dotplot.rs:384-423 through the csv writer of render_output) ------------------------------------------
 * d_counts[n] are wga_cigar_stat's or wga_maf_pair_stat's counters; d_heads[n] the four numbers AS PRINTED (the caller has
 * swapped the query pair of a `-` record), the divisor and the spans of the two names inside d_names[0 .. n_name_bytes).
 * Row r, in input order, is ONE line of 7 columns, commas between them:
 *   <ref_start>,<ref_end>,<q_first>,<q_second>,<identity>,<ref_chro>,<query_chro>\n
 *   identity = (double)d_counts[r].match / (double)align_size
 * u64 -> f64 rounds to nearest even and the division is the IEEE double precision one: 0 / 0 prints "NaN", x / 0 "inf".  With
 * no_identity != 0 the column is the literal "1.0", d_counts may be NULL and nothing is read from it.  Integers are printed in
 * canonical decimal.  A name is written as the csv writer does under QuoteStyle::Necessary with a comma delimiter (as it is,
 * unless it holds a comma, a quote, CR or LF: then between quotes, every quote inside doubled); a name whose span does not lie
 * inside d_names is written as empty.  An f64 is written as ryu does (wga_f64_text below).
 *   d_out == NULL: the byte count of every row (d_work), d_row_off[n + 1] (device memory; d_row_off[n] = the text's length)
 *                  and *total_bytes (a host value; the call synchronises).
 *   otherwise    : the text at d_out[0 .. *total_bytes).  d_out may have any alignment, the caller leaves 16 bytes of slack
 *                  behind the text; no byte in front of d_out and none from d_out + *total_bytes on is written.  *total_bytes,
 *                  d_work and d_row_off are read as the first call left them, so the two calls take the same arguments.  A row
 *                  whose span in d_row_off is not its byte count in d_work is not written.
 * All places are 64-bit.  n == 0: *total_bytes = 0, nothing is written.  WGA_E_INVALID_ARG: a null d_work or total_bytes,
 * whatever n; a null array with n > 0 (d_counts only when !no_identity, d_names only when n_name_bytes > 0); n > 0xFFFFFFF0.
 * d_work: wga_dotplot_overview_work_bytes(n) bytes of device memory, 8-byte aligned, shared by the two calls
 * = 8 * (n + n / 1024 + 4): 8 bytes per row for its byte count, plus the scan's partial sums (32 bytes for n == 0). */
typedef struct {
  uint64_t ref_start, ref_end, q_first, q_second;          /* as printed */
  uint64_t align_size;                                      /* the divisor of identity */
  uint64_t rname_off, qname_off;                            /* spans of d_names */
  uint32_t rname_len, qname_len;
} wga_dotplot_ov_head;                                      /* 64 bytes */

uint64_t wga_dotplot_overview_work_bytes(uint64_t n);
int wga_dotplot_overview(wga_ctx*, uint32_t n, const uint8_t* d_names, uint64_t n_name_bytes,
                         const wga_dotplot_ov_head* d_heads, const wga_cigar_counts* d_counts, int no_identity,
                         void* d_work, uint64_t* d_row_off /* n + 1, device */, uint64_t* total_bytes, uint8_t* d_out);

/* the formatter alone, for tests: d_text[32 i ..] receives the text of the f64 with bit pattern d_bits[i], d_len[i] its length
 * (at most 24; the bytes of d_text behind a text are left as they were).  NaN -> "NaN", +-inf -> "inf" / "-inf", +-0 -> "0.0" /
 * "-0.0", anything else the shortest digits that read back as the same f64, the closest such to the value, laid out as
 * ryu::Buffer::format does: with the digits' count len, the decimal exponent k of the last digit and kk = len + k
 *   0 <= k && kk <= 16 : digits, k zeros, ".0"         0 < kk <= 16 : dddd.ddd
 *   -5 < kk <= 0       : "0.", -kk zeros, digits       else         : d[.ddd]e<kk - 1>
 * n == 0 is valid; WGA_E_INVALID_ARG: a null array with n > 0, n > 0xFFFFFFF0. */
int wga_f64_text(wga_ctx*, uint64_t n, const uint64_t* d_bits, uint8_t* d_text /* 32 n bytes */, uint8_t* d_len);

/* ---- K35: `maf-index` — block offsets, name groups and the JSON interval text (replaces, for a piece the device splitter took,
 *      the second walk over the file for the blocks' offsets, the host records and the per-s-line map lookup and append of
 *      cmd_maf_index, wgatools_amd/host/cmd_ext.inc; in the reference tools/index.rs:14-94) ------------------------------------
 * d_text, n_bytes, d_lines[n_lines]: the arguments and the result of wga_maf_split, with its limits.  skip = 0, or 2 for a piece
 * that starts with the dummy line "#\n"; base = the file position of d_text[skip]; carry_offset = the position behind the last
 * record-ending line seen before this piece.
 * Blocks and offsets.  A block is a maximal run of WGA_MAF_SLINE lines.  Its offset is the file position behind the '\n' of the line
 * that ended the run in front of it (the first line behind that run that is not an s-line; lines skipped in front of a run's first
 * s-line lie inside the block's span); a record-ending line without a final '\n' ends at n_bytes.  The piece's first block takes the
 * end of the piece's first line when skip == 0 (the file's header line, whatever it starts with), otherwise carry_offset.
 * *next_offset = the carry for the next piece: the position behind the last line of the piece that ended a run — where the piece's
 * last run has no ending line, or the piece has no run, the value its last block took or would have taken (so carry_offset itself
 * for a piece with skip == 2 that ends no run).
 * Name groups.  Two s-lines belong to the same group exactly when their name bytes are equal: a hash only places a name in the
 * table, the bytes decide.  Groups are numbered by ascending first s-line.  Context parameter "maf_index_hash_bits" (1 .. 64,
 * default 64): the hash is cut to that many low bits, so that a test makes every name collide.  Within a group the intervals stand
 * in file order: a stable LSD radix sort of the s-lines by group number, in as many passes as the group count has digits of
 * "maf_index_sort_bits" bits (1 .. 8, default 8; any width gives the same order).
 * Errors of the reference, as line indices (WGA_NONE when absent; both by atomicMin, so runs agree):
 *   *first_dup_line       the lowest s-line whose name occurs earlier in the same block (index.rs:33-37)
 *   *first_conflict_line  the lowest s-line whose isref — being the first line of its run — differs from that of its group's
 *                         first line (index.rs:54-58)
 * Output.  d_names[*n_names + 1]: one entry per group — the name's span in d_text, size (num[2] of the group's first line),
 * first_line, isref, n_ivls and text_off, the place of the group's text in d_out — and a closing entry with text_off =
 * *text_bytes and zeros.  d_out[0 .. *text_bytes): the interval text group after group, a group's intervals joined by ',' and
 * without brackets, an interval
 *   {"start":S,"end":E,"strand":"+","offset":O}            ("-" for a line on the '-' strand)
 * with S = num[0], E = num[0] + num[1] mod 2^64 and O the block's offset, in canonical decimal.
 *   d_names == NULL and d_out == NULL: everything but the table and the text; *n_names, *n_blocks, *n_slines, *text_bytes,
 *                  the two error lines and *next_offset are host values (the call synchronises).
 *   otherwise    : the table and the text.  d_out may have any alignment, the caller leaves 16 bytes of slack behind the text; no
 *                  byte in front of d_out and none from d_out + *text_bytes on is written.  The counts and d_work are read as
 *                  the first call left them, so the two calls take the same arguments.
 * All places are 64-bit.  n_lines == 0 or a table without an s-line: the counts are zero, the call succeeds, nothing is written.
 * WGA_E_FALLBACK: the table holds a WGA_MAF_FALLBACK line (the caller reads the piece with its host reader).  WGA_E_INVALID_ARG:
 * a null d_work or host pointer, whatever n_lines; a null array or n_bytes == 0 with n_lines > 0; n_lines that is not the text's
 * line count; a text beyond wga_maf_split's limits; skip other than 0 and 2; a second call with a null d_names or d_out.
 * d_work: wga_maf_index_work_bytes(n_lines) bytes of device memory, 8-byte aligned, shared by the two calls. */
typedef struct {
  uint64_t name_off;    /* the name's span in d_text */
  uint64_t size;        /* num[2] of the group's first line */
  uint64_t first_line;  /* the group's first s-line: an index into d_lines */
  uint64_t n_ivls;
  uint64_t text_off;    /* the group's text is d_out[text_off, the next entry's text_off) */
  uint32_t name_len;
  uint32_t isref;
} wga_maf_index_name;   /* 48 bytes */

uint64_t wga_maf_index_work_bytes(uint64_t n_lines);
int wga_maf_index(wga_ctx*, const uint8_t* d_text, uint64_t n_bytes, const wga_maf_line* d_lines, uint64_t n_lines, uint32_t skip,
                  uint64_t base, uint64_t carry_offset, void* d_work, uint64_t* n_names, uint64_t* n_blocks, uint64_t* n_slines,
                  uint64_t* text_bytes, uint64_t* first_dup_line, uint64_t* first_conflict_line, uint64_t* next_offset,
                  wga_maf_index_name* d_names /* *n_names + 1, device */, uint8_t* d_out);

/* ---- K36: `stat` — the merged table (replaces, without `-e`, the download of every record's counters, the two strings per record
 *      kept to the end of the file, the map lookup per record and the thirteen additions per record of stat_tsv,
 *      wgatools_amd/host/wga_host.cpp; in the reference the Pair aggregation of merge_final_from_pair stat.rs:167-223) -----------
 * wga_stat_pairs takes wga_stat_rows' inputs: d_heads[n] with the four numbers as printed and the spans of the two names inside
 * d_names[0 .. n_name_bytes) (a span that does not lie inside counts as the empty name), d_counts[n] wga_cigar_stat's or
 * wga_maf_pair_stat's counters.
 * Pairs.  Two records are one pair exactly when their ref_name bytes, ref_size, query_name bytes and query_size agree: a hash only
 * places a record in the table, the bytes and the two sizes decide (("ab","c") and ("a","bc") are two pairs, and so are equal names
 * with different sizes).  Pairs are numbered by ascending first_rec, the first-appearance order.  Context parameter
 * "stat_pair_hash_bits" (1 .. 64, default 64): the hash is cut to that many low bits, so that a test makes every pair collide.
 * Of pair p, with all integer arithmetic mod 2^64:
 *   first_rec, n_recs        its lowest record (whose head holds the names and sizes) and how many it has
 *   ref_start, query_start   min(ref_size, min ref_start), min(query_size, min query_start): stat.rs:186-213
 *   sum                      each of the eleven counters, summed (stat.rs:194-205; aligned_size is match + mismatch + del_bp +
 *                            inv_del_bp of the sums)
 *   inv_size_bits            the bits of an f32: the left fold, in ascending record order, of the values
 *                            (float)(aligned + query_align) / (float)(inv_ev + 1) (wga_stat_rows' inv_size) of the pair's records
 *                            with inv_ev != 0, from the start value d_inv_in[p] (an f32's bits; d_inv_in == NULL: +0.0).  This
 *                            is stat.rs:206 in input order: adding the other records' +0.0 changes nothing.
 *   d_pairs == NULL and d_pair_of_rec == NULL: the grouping is built in d_work and *n_pairs, a host value, is set (the call
 *                  synchronises).
 *   otherwise    : d_pair_of_rec[n] and d_pairs[*n_pairs] are written; cap_pairs >= *n_pairs (WGA_E_TOO_SMALL otherwise).
 *                  *n_pairs and d_work are read as the first call left them, so the two calls take the same arguments.  The call
 *                  may be repeated on the same outputs with another d_inv_in: it then rewrites inv_size_bits alone.
 * n == 0: *n_pairs = 0, nothing is written.  WGA_E_INVALID_ARG: a null d_work or n_pairs, whatever n; a null array with n > 0
 * (d_names only when n_name_bytes > 0; one of the two outputs without the other); n > 0xFFFFFFF0; an *n_pairs that is not the first
 * call's.
 * d_work: wga_stat_pairs_work_bytes(n) bytes of device memory, 8-byte aligned, shared by the calls
 * = 8 * (8 + M + 2 * (n + 1) + C + n / 1024 + C / 1024 + 8) + 4 * (6 * n + 2), rounded up to a multiple of 8, with M the table's
 * slots (the power of two from 16 to 2^32 that first reaches 2 n) and C = 256 * ((n + 1023) / 1024) + 1 the sort's counters. */
typedef struct {
  uint64_t first_rec, n_recs;        /* lowest record of the pair (its head holds names and sizes); how many */
  uint64_t ref_start, query_start;   /* min(ref_size, min ref_start), min(query_size, min query_start): stat.rs:186-213 */
  wga_cigar_counts sum;              /* each of the 11 counters, summed mod 2^64 */
  uint32_t inv_size_bits, pad;       /* f32, see above */
} wga_stat_pair;                     /* 128 bytes */

uint64_t wga_stat_pairs_work_bytes(uint64_t n);
int wga_stat_pairs(wga_ctx*, uint32_t n, const uint8_t* d_names, uint64_t n_name_bytes, const wga_stat_row_head* d_heads,
                   const wga_cigar_counts* d_counts, void* d_work, uint64_t* n_pairs,
                   uint32_t* d_pair_of_rec, const uint32_t* d_inv_in, wga_stat_pair* d_pairs, uint64_t cap_pairs);

/* the pairs' rows (stat.rs:216-218 through the csv writer of stat.rs:117-123): wga_stat_rows over d_sums[n], with its protocol,
 * limits, errors and d_work (wga_stat_rows_work_bytes(n)), d_heads[r] holding pair r's two sizes, its two minima and its names.
 * Row r has wga_stat_rows' 22 columns with two differences: column 8 (unaligned_size) is ref_size - aligned_size mod 2^64, the
 * release build's wrapping difference, and column 18 (inv_size) is the f32 with the bits d_inv_bits[r].  identity and similarity
 * come from the sums by wga_stat_rows' formulas; 0 / 0 prints "NaN".  d_inv_bits is one of the arrays that may not be null
 * with n > 0. */
int wga_stat_pair_rows(wga_ctx*, uint32_t n, const uint8_t* d_names, uint64_t n_name_bytes, const wga_stat_row_head* d_heads,
                       const wga_cigar_counts* d_sums, const uint32_t* d_inv_bits, void* d_work,
                       uint64_t* d_row_off /* n + 1, device */, uint64_t* total_bytes, uint8_t* d_out);

#ifdef __cplusplus
}
#endif
#endif /* WGA_HIP_H */
