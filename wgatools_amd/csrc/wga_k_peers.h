/*
 * wga_k_peers.h — the kernel of the multi-GPU counter reduction (wga_reduce_scatter_i32, capi_multigpu.inc).
 */
#ifndef WGA_K_PEERS_H
#define WGA_K_PEERS_H

#include "wga_kernels.h"

/* dst[i] += the sum of src[k][i] over up to WGA_PEER_MAX source arrays (n counters).
 * The sources are the other devices' buffers, read where they lie (peer access over xGMI: one load per source and thread in
 * flight, so a device's links all carry data at the same time) or, staged, copies of them in this device's scratch.  16 bytes
 * per thread and source where the pointers share their alignment; a grid-stride loop. */
#define WGA_PEER_MAX 15
struct wga_peer_srcs {
  const int* p[WGA_PEER_MAX];
};
__global__ __launch_bounds__(256) void k_add_peers_i32(int* __restrict__ dst, wga_peer_srcs srcs, int n_src, u64 n) {
  const u64 tid = (u64)blockIdx.x * 256u + threadIdx.x, stride = (u64)gridDim.x * 256u;
  bool together = true; /* dst and every source at the same offset inside their 16-byte groups */
  for (int k = 0; k < n_src; k++) together = together && ((((u64)srcs.p[k]) ^ (u64)dst) & 15ull) == 0ull;
  u64 head = together ? ((16ull - ((u64)dst & 15ull)) & 15ull) >> 2 : n; /* counters in front of the first whole group */
  if (head > n) head = n;
  const u64 groups = (n - head) >> 2, tail0 = head + (groups << 2);
  for (u64 q = tid; q < groups; q += stride) {
    const u64 i = head + (q << 2);
    u32x4_a16 acc = *(const u32x4_a16*)(dst + i);
    u32x4_a16 v[WGA_PEER_MAX];
#pragma unroll
    for (int k = 0; k < WGA_PEER_MAX; k++)
      if (k < n_src) v[k] = *(const u32x4_a16*)(srcs.p[k] + i); /* all of them requested before the first is added */
#pragma unroll
    for (int k = 0; k < WGA_PEER_MAX; k++)
      if (k < n_src) acc += v[k];
    *(u32x4_a16*)(dst + i) = acc;
  }
  for (u64 i = tid; i < n - (groups << 2); i += stride) { /* the counters outside whole groups */
    const u64 j = i < head ? i : tail0 + (i - head);
    int acc = dst[j];
    for (int k = 0; k < n_src; k++) acc += srcs.p[k][j];
    dst[j] = acc;
  }
}

#endif /* WGA_K_PEERS_H */
