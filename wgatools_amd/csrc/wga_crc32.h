/*
 * wga_crc32.h — CRC-32 as the gzip trailer holds it, for the kernels that make BGZF members (K18) and that check them (K17's
 * companion k_bgzf_crc32): the tables, and the arithmetic that folds the CRCs of the pieces of a range into the CRC of the range.
 */
#ifndef WGA_CRC32_H
#define WGA_CRC32_H

#include "wga_kernels.h"

/* CRC-32 (reflected 0xEDB88320) tables made at compile time: the byte table, and x^(2^k) mod P for the zero-feeding
 * products that fold partial CRCs (the same arithmetic as zlib's crc32_combine) */
struct wga_crc_tables {
  u32 byte[256];    /* the byte table */
  u32 by4[3][256];  /* its three companions for four bytes at a time (slicing-by-4: by4[k][i] = byte i followed by k + 1 zero bytes) */
  u32 x2n[32];
  static constexpr u32 mul(u32 a, u32 b) {
    u32 m = 1u << 31, p = 0;
    for (;;) {
      if (a & m) {
        p ^= b;
        if ((a & (m - 1u)) == 0u) break;
      }
      m >>= 1;
      b = (b & 1u) ? (b >> 1) ^ 0xEDB88320u : b >> 1;
    }
    return p;
  }
  constexpr wga_crc_tables() : byte{}, by4{}, x2n{} {
    for (u32 i = 0; i < 256u; i++) {
      u32 c = i;
      for (int k = 0; k < 8; k++) c = (c & 1u) ? (c >> 1) ^ 0xEDB88320u : c >> 1;
      byte[i] = c;
    }
    for (u32 i = 0; i < 256u; i++) {
      u32 c = byte[i];
      for (int k = 0; k < 3; k++) by4[k][i] = c = byte[c & 0xFFu] ^ (c >> 8);
    }
    u32 p = 1u << 30; /* x^1 */
    x2n[0] = p;
    for (int k = 1; k < 32; k++) x2n[k] = p = mul(p, p);
  }
};
__device__ const wga_crc_tables k_crc_tables{};

__device__ __forceinline__ u32 crc_mul(u32 a, u32 b) {
  u32 p = 0;
  for (int k = 31; k >= 0; k--) { /* a's bit 31 is x^0 */
    p ^= (0u - ((a >> k) & 1u)) & b;
    b = (b >> 1) ^ ((0u - (b & 1u)) & 0xEDB88320u);
  }
  return p;
}
/* the CRC register after `n_bytes` zero bytes went through it (n_bytes < 2^29) */
__device__ __forceinline__ u32 crc_shift(u32 crc, u32 n_bytes) {
  u32 k = 3; /* x^(8 n) */
  while (n_bytes) {
    if (n_bytes & 1u) crc = crc_mul(k_crc_tables.x2n[k], crc);
    n_bytes >>= 1;
    k++;
  }
  return crc;
}

#endif /* WGA_CRC32_H */
