/*
 * wga_text_out.h — what the kernels that write text share: decimal numbers, the count / put sink pair, the staged stretch and
 * its flush, the bisection that finds an element's record, the fill kernel of the texts that are a stream of items, and the
 * skeleton of the texts that are one row per record (both at the end of the file).  Nothing here knows a format.
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
  u64 n = 0;
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

/* ITEM STREAMS.  A text that is ONE contiguous byte stream of variable-size items (K25's and K27's heads and lines, K28's heads
 * and runs, K26's rows) is sized by a scan over ScanItems<F> and written by k_text_items_fill<F>, 256 consecutive items per block =
 * one contiguous stretch, whatever record borders lie inside it.  The format F is a plain struct passed by value:
 *   static constexpr u32 kStage            the bytes of a block's stretch that go through LDS (a longer one is written directly)
 *   static constexpr bool kCheckSize       the fill compares size(x, r) with the scan's span before it writes item x
 *   u32 n_rec                              records
 *   u32 rec(u64 x, u32 lo, u32 hi) const   the record of item x, known to lie in [lo, hi): csr_find_in over F's offsets
 *   u64 size(u64 x, u32 r) const           the bytes of item x of record r: its emitter into a TextCount
 *   void emit(S& s, u64 x, u32 r) const    the emitter */
#define WGA_TEXT_ITEMS 256u

template <typename F>
struct ScanItems { /* scan functor: the bytes of item x */
  F f;
  __device__ u64 operator()(u32 x) const { return f.size((u64)x, f.rec((u64)x, 0u, f.n_rec)); }
};

/* items [256 b, 256 b + 256) of n_items; isc = the exclusive scan of their sizes (isc[n_items] = the text's length).  ONE GUARD
 * for a scan that is not this call's: a block whose stretch ends behind `total` writes nothing, and an item is written only into
 * a span [isc[x], isc[x + 1]) that is not empty and lies inside the block's stretch — and, where F::kCheckSize is set, has the
 * size the emitter is about to write: then nothing is written outside out[0, total) and nothing into a span but its item's text,
 * whatever the scan holds.  Without it (K25, K27, and K28 after them: their fills cannot pay a second walk over an item's digits,
 * profiles/text_items_refactor.txt) an item longer than its span runs on into the bytes behind it, as it always did there.
 * A span that is refused keeps its bytes: in a staged block its thread copies what memory holds there into the stage and the
 * flush puts it back (the intervals between isc[x] and isc[x + 1] cover the stretch whatever the scan holds, so every byte of the
 * stage is some item's text or what memory held; where a scan that does not ascend lays a refused span over a written item's,
 * which of the two lands in a byte that both cover is not determined). */
template <typename F>
__global__ __launch_bounds__(256) void k_text_items_fill(F f, u64 n_items, const u64* __restrict__ isc, u64 total,
                                                         u8* __restrict__ out) {
  __shared__ u32x4_a16 s_buf[(F::kStage + 32u) / 16u];
  __shared__ u32 s_r[2];
  const u32 tid = threadIdx.x;
  const u64 x0 = (u64)blockIdx.x * WGA_TEXT_ITEMS;
  const u64 x1 = x0 + WGA_TEXT_ITEMS < n_items ? x0 + WGA_TEXT_ITEMS : n_items;
  const u64 e0 = isc[x0], e1 = isc[x1]; /* bytes in front of the block, and behind it */
  if (e1 <= e0 || e1 > total) return;   /* block-uniform: nothing to write (K25: every chain of the block is dropped) */
  if (tid < 2u) s_r[tid] = f.rec(tid ? x1 - 1u : x0, 0u, f.n_rec); /* the records of the first and the last item */
  __syncthreads();
  const TextStretch st(s_buf, F::kStage, out + e0, e1 - e0); /* block-uniform */
  const u64 x = x0 + tid;
  if (x < x1) {
    const u64 at = isc[x], end = isc[x + 1u];
    bool put = at >= e0 && end <= e1 && end > at;
    if (F::kCheckSize || put) {
      const u32 r = f.rec(x, s_r[0], s_r[1] + 1u);
      if (F::kCheckSize) put = (end - at == f.size(x, r)) && put; /* the size first: its reads go with the scan's */
      if (put) {
        TextPut w = {st.at(at - e0)};
        f.emit(w, x, r);
      }
    }
    if (!put && end != at && st.staged) { /* end == at: an item without bytes (K25: of a dropped chain) */
      const u64 lo = at < end ? at : end, hi = at < end ? end : at; /* the span, and of it what lies in the stretch */
      for (u64 k = lo > e0 ? lo : e0; k < (hi < e1 ? hi : e1); k++) *st.at(k - e0) = out[k];
    }
  }
  st.flush_block(tid);
}

/* RECORD ROWS.  A text of one row per record (K33's TSV rows, K34's csv rows) is the item stream whose item x is row x of record
 * x.  The row source R is a plain struct passed by value:
 *   static constexpr u32 kStage            as above
 *   names, n_name_bytes, heads, counts     what the rows are made of (four fields: the kernel arguments' layout hangs on it)
 *   void emit(S& s, u32 r) const           row r's emitter
 *   plan   k_record_rows_plan<R>: one thread per row, the emitter into a TextCount.
 *   scan   ScanItems<F> over the plan, F a struct derived from RecordRowsFmt<R>, into the caller's row_off[n + 1].
 *   fill   k_text_items_fill<F>.  kCheckSize is on and costs one load: the size of a row is its plan, so a row_off that is not
 *          this plan's scan is not written into. */
template <typename R>
struct RecordRowsFmt : R {
  using Src = R;
  static constexpr bool kCheckSize = true;
  const u64* plan;
  u32 n_rec;
  __device__ __forceinline__ u32 rec(u64 x, u32, u32) const { return (u32)x; }
  __device__ __forceinline__ u64 size(u64, u32 r) const { return plan[r]; }
  template <typename S>
  __device__ __forceinline__ void emit(S& s, u64, u32 r) const {
    R::emit(s, r);
  }
};

/* plan[r] = the bytes of row r; the source's four fields as arguments of their own */
template <typename R>
__global__ __launch_bounds__(256) void k_record_rows_plan(const u8* __restrict__ names, u64 n_name_bytes,
                                                          decltype(R::heads) __restrict__ heads, u32 n,
                                                          decltype(R::counts) __restrict__ counts, u64* __restrict__ plan) {
  const u64 r = (u64)blockIdx.x * 256u + threadIdx.x;
  if (r >= (u64)n) return;
  const R src = {names, n_name_bytes, heads, counts};
  TextCount t;
  src.emit(t, (u32)r);
  plan[r] = t.n;
}

/* A formatter alone (K33's f32, K34's f64): text[kSlot i ..) = the text of the value with the bits bits[i], len[i] its length; the
 * bytes behind a text are left as they were */
template <typename B, u32 kSlot, void (*kEmit)(TextPut&, B)>
__global__ __launch_bounds__(256) void k_bits_text(u64 n, const B* __restrict__ bits, u8* __restrict__ text, u8* __restrict__ len) {
  const u64 i = (u64)blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  TextPut w = {text + kSlot * i};
  kEmit(w, bits[i]);
  len[i] = (u8)(w.p - (text + kSlot * i));
}

#endif /* WGA_TEXT_OUT_H */
