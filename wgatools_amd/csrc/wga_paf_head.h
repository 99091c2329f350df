/* wga_paf_head.h — what the kernels that write PAF records share (K27, K28): a name as the csv writer prints it, and the twelve
 * columns with the tags in front of the CIGAR text. */
#ifndef WGA_PAF_HEAD_H
#define WGA_PAF_HEAD_H

#include "wga_text_out.h" /* the sinks */

/* a field as the csv writer writes it under QuoteStyle::Necessary: as it is, unless it holds the delimiter, a quote, CR or LF;
 * then between quotes with every quote inside doubled */
template <u8 kDelim, typename S>
__device__ __forceinline__ void csv_field_emit(S& s, const u8* __restrict__ p, u32 len) {
  bool need = false;
  for (u32 k = 0; k < len && !need; k++) {
    const u8 b = p[k];
    need = b == kDelim || b == (u8)'"' || b == (u8)'\n' || b == (u8)'\r';
  }
  if (!need) {
    s.str(p, len);
    return;
  }
  s.c((u8)'"');
  for (u32 k = 0; k < len; k++) {
    const u8 b = p[k];
    if (b == (u8)'"') s.c(b);
    s.c(b);
  }
  s.c((u8)'"');
}

/* the twelve columns of a PAF record whose CIGAR follows, up to and including the tag's name; q / t = size, start, end.
 * kNm: "NM:i:<block_length - matches>" (wrapping) stands in front of the cg tag (maf2paf: maf.rs:484-520) */
template <bool kNm = false, typename S>
__device__ __forceinline__ void paf_head_emit(S& s, const u8* __restrict__ qname, u32 qname_len, const u64* q, bool neg,
                                              const u8* __restrict__ tname, u32 tname_len, const u64* t, u64 matches,
                                              u64 block_length, u64 mapq) {
  csv_field_emit<(u8)'\t'>(s, qname, qname_len);
  for (u32 k = 0; k < 3u; k++) {
    s.c((u8)'\t');
    s.dec(q[k]);
  }
  s.c((u8)'\t');
  s.c(neg ? (u8)'-' : (u8)'+');
  s.c((u8)'\t');
  csv_field_emit<(u8)'\t'>(s, tname, tname_len);
  for (u32 k = 0; k < 3u; k++) {
    s.c((u8)'\t');
    s.dec(t[k]);
  }
  s.c((u8)'\t');
  s.dec(matches);
  s.c((u8)'\t');
  s.dec(block_length);
  s.c((u8)'\t');
  s.dec(mapq);
  if (kNm) {
    const char* nm = "\tNM:i:";
    for (u32 k = 0; k < 6u; k++) s.c((u8)nm[k]);
    s.dec(block_length - matches);
  }
  const char* c = "\tcg:Z:";
  for (u32 k = 0; k < 6u; k++) s.c((u8)c[k]);
}

/* the span [off, off + len) of a name buffer of n_bytes: its length, or 0 when it does not lie inside (arrays that are not a
 * splitter's: the name is empty) */
__device__ __forceinline__ u32 name_span_len(u64 off, u32 len, u64 n_bytes) {
  return off <= n_bytes && (u64)len <= n_bytes - off ? len : 0u;
}

#endif /* WGA_PAF_HEAD_H */
