/*
 * wga_k9_bed.h — K9: pafcov BED text (pafcov.rs:56-60).
 * One header per kernel family; wga_capi.cpp includes them in dependency order (a header may use helpers of the ones in front of it).
 */
#ifndef WGA_K9_BED_H
#define WGA_K9_BED_H

#include "wga_text_out.h"

/* ============================================================================================ */
/* K9: pafcov BED text                                                                          */
/* ============================================================================================ */
/* pafcov prints one line per target base, "<name>\t<pos>\t<pos+1>\t<count>\n" (pafcov.rs:56-60):
 * pure formatting, and the bulk of the tool's wall time.  One emitter (wga_text_out.h): counted, it is the
 * scan functor's line length; put, it is the line one thread writes. */
template <typename S>
__device__ __forceinline__ void bed_emit(S& s, const u8* __restrict__ name, u32 name_len, u64 pos, u32 count) {
  s.str(name, name_len);
  s.c((u8)'\t');
  s.dec(pos);
  s.c((u8)'\t');
  s.dec(pos + 1);
  s.c((u8)'\t');
  s.dec((u64)count);
  s.c((u8)'\n');
}
struct ScanCovLine {
  const int* cov;
  u64 p0;
  u32 name_len;
  __device__ u64 operator()(u32 i) const {
    TextCount c;
    c.n = 0;
    bed_emit(c, nullptr, name_len, p0 + i, (u32)cov[i]);
    return c.n;
  }
};
/* A block takes WGA_BED_LINES consecutive lines — one contiguous stretch of the text, staged and flushed as wga_text_out.h
 * describes: a thread per line writing its ~28 bytes one by one to memory was 0.53 TB/s of text (rounds 1-5).  The stage holds
 * 512 lines of names up to ~30 bytes. */
#define WGA_BED_LINES 512u
#define WGA_BED_STAGE 24576u
__global__ __launch_bounds__(256) void k_pafcov_format(ScanCovLine f, u32 n, const u8* __restrict__ name,
                                                       const u64* __restrict__ line_off,
                                                       u8* __restrict__ out) {
  __shared__ u32x4_a16 s_buf[(WGA_BED_STAGE + 32u) / 16u];
  const u32 tid = threadIdx.x;
  const u32 x0 = blockIdx.x * WGA_BED_LINES, x1 = x0 + WGA_BED_LINES < n ? x0 + WGA_BED_LINES : n;
  const u64 first = line_off[0], e0 = line_off[x0], e1 = line_off[x1];
  const TextStretch st(s_buf, WGA_BED_STAGE, out + (e0 - first), e1 - e0); /* block-uniform */
  for (u32 x = x0 + tid; x < x1; x += 256u) {
    TextPut w;
    w.p = st.at(line_off[x] - e0);
    bed_emit(w, name, f.name_len, f.p0 + x, (u32)f.cov[x]);
  }
  st.flush_block(tid);
}

#endif /* WGA_K9_BED_H */
