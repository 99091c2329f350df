/*
 * wga_scan.h — the generic exclusive scan of n u64 values: three kernels, 1024 values per block.  The values come from a
 * functor (ScanPlain: an array; ScanLayout, ScanItems, ... : a family's own sizes), so that every count -> fill launcher
 * instantiates the same kernels (run_scan in wga_capi.cpp).
 */
#ifndef WGA_SCAN_H
#define WGA_SCAN_H

#include "wga_kernels.h"

struct ScanPlain {
  const u64* in;
  __device__ u64 operator()(u32 i) const { return in[i]; }
};

template <typename F>
__global__ __launch_bounds__(256) void k_scan_partials(F f, u32 n, u64* partial) {
  __shared__ u64 s_w[5];
  u32 base = blockIdx.x * 1024u + threadIdx.x * 4u;
  u64 v = 0;
  for (u32 e = 0; e < 4; e++)
    if (base + e < n) v += f(base + e);
  u64 tot;
  (void)block_excl_scan_u64(v, s_w, &tot);
  if (threadIdx.x == 0) partial[blockIdx.x] = tot;
}

/* single block: exclusive scan of nb partials in place, grand total to *total_out */
__global__ __launch_bounds__(256) void k_scan_top(u64* partial, u32 nb, u64* total_out) {
  __shared__ u64 s_w[5];
  u64 carry = 0;
  for (u32 base = 0; base < nb; base += 256u) {
    u32 i = base + threadIdx.x;
    u64 v = i < nb ? partial[i] : 0;
    u64 tot;
    u64 ex = block_excl_scan_u64(v, s_w, &tot);
    if (i < nb) partial[i] = carry + ex;
    carry += tot;
  }
  if (threadIdx.x == 0) *total_out = carry;
}

template <typename F>
__global__ __launch_bounds__(256) void k_scan_final(F f, u32 n, const u64* partial, u64* out) {
  __shared__ u64 s_w[5];
  u32 base = blockIdx.x * 1024u + threadIdx.x * 4u;
  u64 x[4];
  u64 v = 0;
  for (u32 e = 0; e < 4; e++) {
    x[e] = (base + e < n) ? f(base + e) : 0;
    v += x[e];
  }
  u64 tot;
  u64 ex = block_excl_scan_u64(v, s_w, &tot) + partial[blockIdx.x];
  for (u32 e = 0; e < 4; e++) {
    if (base + e < n) out[base + e] = ex;
    ex += x[e];
  }
}

#endif /* WGA_SCAN_H */
