/*
 * wga_text_out.h — what the kernels that write text share: decimal numbers, the count / put sink pair, the staged stretch and
 * its flush, and the bisection that finds an element's record.  Nothing here knows a format or a kernel.
 *
 * ONE EMITTER, TWO SINKS.  A format is one function template `xxx_emit(S& s, ...)` that names its bytes in order through
 * s.c / s.dec / s.str.  Run into a TextCount it is the size the scan adds up, run into a TextPut it is the text: what the count
 * pass adds up is what the fill pass writes, by construction.
 *
 * THE STAGED STRETCH.  A block (or a wave) that owns one contiguous stretch of the output assembles it in an LDS image that
 * mirrors the stretch's place inside its 16-byte group, and the image leaves in 16-byte stores (TextStretch, lds_text_flush).  A
 * stretch longer than the stage is written where it belongs, byte by byte: correct, slow and rare.  The `__shared__` array and
 * its size are the kernel's: it declares the stage and hands it in.
 */
#ifndef WGA_TEXT_OUT_H
#define WGA_TEXT_OUT_H

#include "wga_kernels.h"

__device__ __forceinline__ u32 dec_digits(u64 v) {
  u32 n = 1;
  if (v >= 10000000000ull) {
    v /= 10000000000ull;
    n += 10;
  }
  u32 w = (u32)v; /* < 10^10 does not fit u32 entirely: handle the top digit */
  if (v >= 1000000000ull) return n + 9u;
  if (w >= 100000000u) return n + 8u;
  if (w >= 10000000u) return n + 7u;
  if (w >= 1000000u) return n + 6u;
  if (w >= 100000u) return n + 5u;
  if (w >= 10000u) return n + 4u;
  if (w >= 1000u) return n + 3u;
  if (w >= 100u) return n + 2u;
  if (w >= 10u) return n + 1u;
  return n;
}
/* writes the decimal digits of v (nd = dec_digits(v)) at p[0 .. nd) */
__device__ __forceinline__ void dec_write(u8* p, u64 v, u32 nd) {
  if (v < 0x100000000ull) {
    u32 w = (u32)v;
    for (u32 k = nd; k-- > 0;) {
      p[k] = (u8)('0' + w % 10u);
      w /= 10u;
    }
  } else {
    for (u32 k = nd; k-- > 0;) {
      p[k] = (u8)('0' + (u32)(v % 10ull));
      v /= 10ull;
    }
  }
}
/* bytes [a, a + total) of an LDS text buffer go to gb + a (gb 16-byte aligned: the buffer mirrors the output's position
 * inside its 16-byte group): whole groups with 16-byte stores, the ragged head and tail (< 16 bytes each) by bytes.
 * `nthr` threads share the work (a wave or a block; the caller synchronises around the call). */
__device__ __forceinline__ void lds_text_flush(const u8* tbuf, u32 a, u32 total, u8* gb, u32 tid, u32 nthr) {
  const u32 end = a + total;
  const u32 g_lo = (a + 15u) >> 4, g_hi = end >> 4; /* whole 16-byte groups [g_lo, g_hi) */
  for (u32 g = g_lo + tid; g < g_hi; g += nthr) *(u32x4_a16*)(gb + 16u * g) = *(const u32x4_a16*)(tbuf + 16u * g);
  const u32 head_end = 16u * g_lo < end ? 16u * g_lo : end;           /* [a, head_end) */
  const u32 tail_beg = 16u * g_hi > head_end ? 16u * g_hi : head_end; /* [tail_beg, end) */
  if (tid < 16u) {
    const u32 x = a + tid;
    if (x < head_end) gb[x] = tbuf[x];
  } else if (tid < 32u) {
    const u32 x = tail_beg + (tid - 16u);
    if (x < end) gb[x] = tbuf[x];
  }
}

/* the two sinks of an emitter */
struct TextCount {
  u64 n;
  __device__ __forceinline__ void c(u8) { n++; }
  __device__ __forceinline__ void dec(u64 v) { n += dec_digits(v); }
  __device__ __forceinline__ void str(const u8*, u32 len) { n += len; }
};
struct TextPut {
  u8* p; /* LDS or memory */
  __device__ __forceinline__ void c(u8 ch) { *p++ = ch; }
  __device__ __forceinline__ void dec(u64 v) {
    const u32 nd = dec_digits(v);
    dec_write(p, v, nd);
    p += nd;
  }
  __device__ __forceinline__ void str(const u8* s, u32 len) {
    for (u32 k = 0; k < len; k++) p[k] = s[k];
    p += len;
  }
};

/* A stretch of `bytes` bytes of text whose first byte belongs at `first`, written by the threads of one block (flush_block) or
 * one wave (flush_wave).  `lds` = the kernel's stage: `stage` + 32 bytes, 16-byte aligned.  All of it is uniform over those
 * threads: every one of them constructs it with the same arguments and calls the flush. */
struct TextStretch {
  u8* tbuf;
  u8* g0;
  u32 a, bytes;
  bool staged;
  __device__ __forceinline__ TextStretch(void* lds, u32 stage, u8* first, u64 n)
      : tbuf((u8*)lds), g0(first), a((u32)((uintptr_t)first & 15u)), bytes((u32)n), staged(n <= (u64)stage) {}
  /* the place of the stretch's byte `rel`: in the stage, or in memory */
  __device__ __forceinline__ u8* at(u64 rel) const { return staged ? tbuf + a + (u32)rel : g0 + rel; }
  __device__ __forceinline__ void flush_block(u32 tid) const {
    if (!staged) return;
    __syncthreads();
    lds_text_flush(tbuf, a, bytes, g0 - a, tid, 256u);
  }
  /* ... and the stage is the wave's own again when this returns */
  __device__ __forceinline__ void flush_wave(u32 lane) const {
    if (!staged) return;
    WGA_WAVE_SYNC();
    lds_text_flush(tbuf, a, bytes, g0 - a, lane, 64u);
    WGA_WAVE_SYNC();
  }
};

/* the largest r in [lo, hi) with off[r] + (bias ? r : 0) <= x, given that lo's key is: the record of element x in CSR offsets
 * (records without elements are stepped over wherever they stand); `bias` for items numbered with one extra per record in
 * front.  Always inside [lo, max(hi, lo + 1)), also for offsets that do not ascend. */
__device__ __forceinline__ u32 csr_find_in(const u64* __restrict__ off, u32 lo, u32 hi, u64 x, bool bias = false) {
  while (lo + 1u < hi) {
    const u32 mid = lo + ((hi - lo) >> 1);
    if (off[mid] + (bias ? (u64)mid : 0ull) <= x) lo = mid; else hi = mid;
  }
  return lo;
}

#endif /* WGA_TEXT_OUT_H */
