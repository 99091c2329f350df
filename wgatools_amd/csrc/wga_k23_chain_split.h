/*
 * wga_k23_chain_split.h — K23: the chain line splitter (the reader of chain.rs:58-73,206-383 for plain files).
 * One header per kernel family; wga_capi.cpp includes them in dependency order (a header may use helpers of the ones in front of it).
 */
#ifndef WGA_K23_CHAIN_SPLIT_H
#define WGA_K23_CHAIN_SPLIT_H

#include "wga_k13_splitters.h"

/* ============================================================================================ */
/* K23: chain line splitter (the nom reader of chain.rs:206-383)            */
/* ============================================================================================ */
/* K14's two lists (k_paf_delims<FILL, 1>: white space, newlines and every byte >= 0x80, with the newlines' ranks) and then one
 * thread per line, twice.  A line's KIND is read off its first six bytes: empty = blank, "chain" + white space = header, anything
 * else = data line.  The count pass adds up the headers and data lines of every 256 lines; their scan gives each block of lines
 * its first chain and its first data-line slot.  The parse pass finds its line's kind again, ranks it inside its block and
 * writes straight to the final slot: a header fills head[chain] and line_off[chain], a data line its three u64 at
 * lines[3 * slot].  Nothing per line is kept between the passes.  A line outside the plain grammar, or in the wrong place
 * (what may follow what is decided from the kind of the line in front), puts its index into *first_bad with atomicMin: the file
 * then is the host reader's (same records, or the reference's exact error text).
 * Workspace: 8 B per delimiter and 8 B per newline (K13's lists: 32 B per "size dt dq" line of about 10 bytes, 16 B per byte of
 * text at the very most, for a file of newlines only) plus 8 B per 256 lines. */
#define WGA_CHAIN_OK 0
#define WGA_CHAIN_FALLBACK 1
#define WGA_CHAIN_BLANK 0u
#define WGA_CHAIN_HEADER 1u
#define WGA_CHAIN_DATA 2u
struct wga_chain_head_dev {
  u64 num[8]; /* score, target size, start, end, query size, start, end, chain id */
  u64 tname_off, qname_off;
  u32 tname_len, qname_len;
  u8 tstrand_neg, qstrand_neg, pad[6];
};

/* the ASCII white space of split_whitespace */
__device__ __forceinline__ bool chain_is_ws(u32 ch) { return ch - 9u <= 4u || ch == 0x20u; }

/* line j = bytes [*s, *e) */
__device__ __forceinline__ void chain_line_span(u64 j, u64 n_bytes, u64 n_newlines, const u64* __restrict__ delims,
                                                const u64* __restrict__ nl_idx, u64* s, u64* e) {
  *s = j ? delims[nl_idx[j - 1]] + 1 : 0;
  *e = j < n_newlines ? delims[nl_idx[j]] : n_bytes;
}

__device__ __forceinline__ u32 chain_line_kind(const u8* __restrict__ text, u64 s, u64 e) {
  if (s == e) return WGA_CHAIN_BLANK;
  if (e - s >= 6u && text[s] == (u8)'c' && text[s + 1] == (u8)'h' && text[s + 2] == (u8)'a' && text[s + 3] == (u8)'i' &&
      text[s + 4] == (u8)'n' && chain_is_ws(text[s + 5]))
    return WGA_CHAIN_HEADER;
  return WGA_CHAIN_DATA;
}

/* headers (low half) and data lines (high half) of line j: both totals stay below 2^32 */
__device__ __forceinline__ u64 chain_kind_count(u32 kind) {
  return kind == WGA_CHAIN_HEADER ? 1ull : kind == WGA_CHAIN_DATA ? 1ull << 32 : 0ull;
}

__global__ __launch_bounds__(256) void k_chain_kinds(const u8* __restrict__ text, u64 n_bytes, u64 n_lines, u64 n_newlines,
                                                     const u64* __restrict__ delims, const u64* __restrict__ nl_idx,
                                                     u64* blk) {
  __shared__ u64 s_w[5];
  const u64 j = (u64)blockIdx.x * 256u + threadIdx.x;
  u64 cnt = 0;
  if (j < n_lines) {
    u64 s, e;
    chain_line_span(j, n_bytes, n_newlines, delims, nl_idx, &s, &e);
    cnt = chain_kind_count(chain_line_kind(text, s, e));
  }
  u64 tot;
  (void)block_excl_scan_u64(cnt, s_w, &tot);
  if (threadIdx.x == 0) blk[blockIdx.x] = tot;
}

/* heads == nullptr: the count call's pass, which only validates */
__global__ __launch_bounds__(256) void k_chain_parse(const u8* __restrict__ text, u64 n_bytes, u64 n_lines, u64 n_newlines,
                                                     u64 n_delims, const u64* __restrict__ delims,
                                                     const u64* __restrict__ nl_idx, const u64* __restrict__ blk_off,
                                                     u64* first_bad, wga_chain_head_dev* heads, u64* lines, u64* line_off) {
  __shared__ u64 s_w[5];
  const u64 j = (u64)blockIdx.x * 256u + threadIdx.x;
  const bool live = j < n_lines;
  u64 s = 0, e = 0;
  u32 kind = WGA_CHAIN_BLANK;
  if (live) {
    chain_line_span(j, n_bytes, n_newlines, delims, nl_idx, &s, &e);
    kind = chain_line_kind(text, s, e);
  }
  u64 tot;
  const u64 at = blk_off[blockIdx.x] + block_excl_scan_u64(live ? chain_kind_count(kind) : 0ull, s_w, &tot);
  if (!live) return;
  const u64 chain = at & 0xFFFFFFFFull, slot = at >> 32;
  /* what may follow what: the first line is a header; a header is followed by a data line; a data line follows a header or a
   * data line; the last line ends in a newline */
  bool ok = j < n_newlines;
  if (j == 0) {
    ok = ok && kind == WGA_CHAIN_HEADER;
  } else {
    u64 ps, pe;
    chain_line_span(j - 1, n_bytes, n_newlines, delims, nl_idx, &ps, &pe);
    const u32 pk = chain_line_kind(text, ps, pe);
    if (kind == WGA_CHAIN_DATA) ok = ok && pk != WGA_CHAIN_BLANK;
    else ok = ok && pk != WGA_CHAIN_HEADER;
  }
  if (kind == WGA_CHAIN_HEADER && j + 1 == n_lines) ok = false; /* a header at the end of the file has no data line */
  /* the line's tokens: its inner delimiters are delims[d0, d1) */
  const u64 d0 = j ? nl_idx[j - 1] + 1 : 0;
  const u64 d1 = j < n_newlines ? nl_idx[j] : n_delims;
  u64 prev = s;
  u32 nt = 0;
  if (kind == WGA_CHAIN_HEADER) {
    wga_chain_head_dev H;
    for (int k = 0; k < 8; k++) H.num[k] = 0;
    H.tname_off = H.qname_off = 0;
    H.tname_len = H.qname_len = 0;
    H.tstrand_neg = H.qstrand_neg = 0;
    for (int k = 0; k < 6; k++) H.pad[k] = 0;
    for (u64 d = d0; d <= d1; d++) {
      const u64 p = d < d1 ? delims[d] : e;
      if (d < d1 && !(text[p] != 0x0Du && text[p] < 0x80u)) ok = false; /* a CR, a byte >= 0x80: anywhere on the line */
      if (p > prev && nt < 13u) { /* a token; surplus ones are ignored (chain.rs:206-322) */
        bool good = true;
        switch (nt) {
          case 0: break; /* "chain" */
          case 1: /* the score: 1 to 15 digits, exact in an f64 */
            good = p - prev <= 15u && text[prev] != (u8)'+' && paf_parse_u64(text, prev, p, &H.num[0]);
            break;
          case 2: H.tname_off = prev; H.tname_len = (u32)(p - prev); break;
          case 3: good = paf_parse_u64(text, prev, p, &H.num[1]); break;
          case 4:
            good = p - prev == 1u && (text[prev] == (u8)'+' || text[prev] == (u8)'-');
            H.tstrand_neg = good && text[prev] == (u8)'-' ? 1 : 0;
            break;
          case 5: good = paf_parse_u64(text, prev, p, &H.num[2]); break;
          case 6: good = paf_parse_u64(text, prev, p, &H.num[3]); break;
          case 7: H.qname_off = prev; H.qname_len = (u32)(p - prev); break;
          case 8: good = paf_parse_u64(text, prev, p, &H.num[4]); break;
          case 9:
            good = p - prev == 1u && (text[prev] == (u8)'+' || text[prev] == (u8)'-');
            H.qstrand_neg = good && text[prev] == (u8)'-' ? 1 : 0;
            break;
          case 10: good = paf_parse_u64(text, prev, p, &H.num[5]); break;
          case 11: good = paf_parse_u64(text, prev, p, &H.num[6]); break;
          default: good = paf_parse_u64(text, prev, p, &H.num[7]); break;
        }
        if (!good) ok = false;
        nt++;
      }
      prev = p + 1;
    }
    if (nt < 13u) ok = false;
    if (heads) {
      heads[chain] = H;
      line_off[chain] = slot;
    }
  } else if (kind == WGA_CHAIN_DATA) {
    u64 v[3] = {0, 0, 0};
    for (u64 d = d0; d <= d1; d++) {
      const u64 p = d < d1 ? delims[d] : e;
      if (d < d1 && !(text[p] != 0x0Du && text[p] < 0x80u)) ok = false;
      if (p > prev) {
        if (nt >= 3u || !paf_parse_u64(text, prev, p, &v[nt < 3u ? nt : 0u])) ok = false; /* a fourth token: nom ignores it */
        nt++;
      }
      prev = p + 1;
    }
    if (nt == 0u) ok = false; /* white space only: "`size` Missing" */
    if (lines) {
      lines[3 * slot] = v[0];
      lines[3 * slot + 1] = v[1];
      lines[3 * slot + 2] = v[2];
    }
  }
  if (!ok) atomicMin(first_bad, j);
}

/* the offsets of chains [first, first + n] as a batch of their own sees them: dst[i] = src[i] - src[0] */
__global__ __launch_bounds__(256) void k_chain_rebase(u32 n, const u64* __restrict__ src, u64* dst) {
  const u64 i = (u64)blockIdx.x * 256u + threadIdx.x;
  if (i <= (u64)n) dst[i] = src[i] - src[0];
}

#endif /* WGA_K23_CHAIN_SPLIT_H */
