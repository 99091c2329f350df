/*
 * wga_f32_text.h — the text of an f32 as the reference's csv writer prints it (ryu::Buffer::format -> pretty::format32): the
 * shortest decimal digits that read back as the same float, the closest such to the value, in ryu's layout.  The host's
 * format_f32 (wga_host.cpp, over std::to_chars) gives the same bytes; scripts/f32_text_exhaustive.py compares the two for all
 * 2^32 bit patterns (profiles/k33_f32_exhaustive.txt).
 *
 * A plain function of the bits: integer arithmetic only, no wave intrinsics, no floating point.  It needs u8 / u32 / u64,
 * `__device__` and `__forceinline__` from whoever includes it (wga_kernels.h in the kernels, three lines in a host program) and
 * writes through a sink with c(u8) and dec(u64) (TextCount / TextPut of wga_text_out.h, or anything alike).
 *
 * THE DIGITS follow Ulf Adams, "Ryu: fast float-to-string conversion" (PLDI 2018), the 32-bit variant: with v = m2 * 2^e2 and
 * the halfway points to its neighbours, vm < vr < vp are those three numbers scaled by a power of ten chosen so that the
 * integer parts hold all the digits that matter; digits are dropped from all three while vp / 10 > vm / 10, and the last dropped
 * digit rounds vr.  The scaling is ONE 32 x 64-bit multiplication and a shift by a table value:
 *   e2 >= 0 : x * 2^e2 / 10^q = x * 2^(e2 - q) / 5^q   -> f32_pow5_inv[q] = floor(2^(bits(5^q) - 1 + 59) / 5^q) + 1
 *   e2 <  0 : x * 5^i / 2^(q ...)                      -> f32_pow5[i]     = the top 61 bits of 5^i
 * The tables are computed here, at compile time, from exact 128-bit integer arithmetic (F32TextTables): 5^i by repeated
 * multiplication (5^47 < 2^110), the reciprocals by binary long division.  bits[i] = the bit length of 5^i.
 */
#ifndef WGA_F32_TEXT_H
#define WGA_F32_TEXT_H

struct F32TextTables {
  u64 pow5[48];     /* 5^i scaled to 61 bits: >> (bits - 61), or << (61 - bits) */
  u64 pow5_inv[31]; /* floor(2^(bits - 1 + 59) / 5^i) + 1 */
  u32 bits[48];     /* the bit length of 5^i (1 for i = 0) */
  u32 pow10[10];
  constexpr F32TextTables() : pow5{}, pow5_inv{}, bits{}, pow10{} {
    unsigned __int128 p = 1;
    for (int i = 0; i < 48; i++) {
      u32 b = 0;
      for (unsigned __int128 t = p; t != 0; t >>= 1) b++;
      bits[i] = b;
      pow5[i] = b >= 61u ? (u64)(p >> (b - 61u)) : (u64)(p << (61u - b));
      if (i < 31) { /* 2^j / p by long division: the remainder stays below p < 2^70 */
        const u32 j = b - 1u + 59u;
        unsigned __int128 rem = p == 1u ? 0u : 1u, quo = p == 1u ? 1u : 0u; /* the numerator's leading one taken */
        for (u32 s = 0; s < j; s++) {
          rem <<= 1;
          quo <<= 1;
          if (rem >= p) {
            rem -= p;
            quo |= 1;
          }
        }
        pow5_inv[i] = (u64)quo + 1u;
      }
      p *= 5u;
    }
    u32 t = 1;
    for (int i = 0; i < 10; i++) {
      pow10[i] = t;
      t *= 10u; /* the last product wraps and is not used */
    }
  }
};
static constexpr F32TextTables kF32Text = F32TextTables();
static_assert(kF32Text.pow5_inv[0] == (1ull << 59) + 1u && kF32Text.pow5[0] == (1ull << 60) && kF32Text.bits[1] == 3u &&
                  kF32Text.pow5[1] == (5ull << 58) && kF32Text.pow10[9] == 1000000000u,
              "the tables of the f32 text");

/* floor(e * log10(2)) for 0 <= e <= 1650, floor(e * log10(5)) for 0 <= e <= 2620 (the paper's fixed-point forms) */
__device__ __forceinline__ u32 f32_log10_pow2(u32 e) { return (e * 78913u) >> 18; }
__device__ __forceinline__ u32 f32_log10_pow5(u32 e) { return (e * 732923u) >> 20; }
/* (m * factor) >> shift, 32 < shift < 96: the result fits 32 bits */
__device__ __forceinline__ u32 f32_mul_shift(u32 m, u64 factor, u32 shift) {
  const u64 lo = (u64)m * (u32)factor, hi = (u64)m * (u32)(factor >> 32);
  return (u32)(((lo >> 32) + hi) >> (shift - 32u));
}
/* 5^p divides v (v != 0) */
__device__ __forceinline__ bool f32_mult_of_pow5(u32 v, u32 p) {
  u32 n = 0;
  while (v % 5u == 0u) {
    v /= 5u;
    n++;
  }
  return n >= p;
}

/* the shortest digits of the finite, non-zero f32 with these mantissa and exponent fields: *digits (1 .. 9 digits, no sign) and
 * the decimal exponent of its LAST digit */
__device__ __forceinline__ void f32_shortest(u32 mant, u32 expo, u32* digits, int* exp10) {
  const int e2 = (expo ? (int)expo : 1) - 127 - 23 - 2;
  const u32 m2 = expo ? (1u << 23) | mant : mant;
  const bool accept = (m2 & 1u) == 0u; /* round to even takes the halfway points in */
  const u32 mv = 4u * m2, mp = 4u * m2 + 2u;
  const u32 mm_shift = (mant != 0u || expo <= 1u) ? 1u : 0u; /* a mantissa of 0: the lower neighbour is half as far */
  const u32 mm = 4u * m2 - 1u - mm_shift;
  u32 vr, vp, vm, last = 0;
  int e10;
  bool vm_tz = false, vr_tz = false; /* all digits dropped so far were 0 */
  if (e2 >= 0) {
    const u32 q = f32_log10_pow2((u32)e2);
    e10 = (int)q;
    const u32 k = 59u + kF32Text.bits[q] - 1u;
    const u32 i = (u32)(-e2 + (int)q + (int)k);
    vr = f32_mul_shift(mv, kF32Text.pow5_inv[q], i);
    vp = f32_mul_shift(mp, kF32Text.pow5_inv[q], i);
    vm = f32_mul_shift(mm, kF32Text.pow5_inv[q], i);
    if (q != 0u && (vp - 1u) / 10u <= vm / 10u) { /* the loop below will not run: the digit it would have dropped */
      const u32 l = 59u + kF32Text.bits[q - 1u] - 1u;
      last = f32_mul_shift(mv, kF32Text.pow5_inv[q - 1u], (u32)(-e2 + (int)q - 1 + (int)l)) % 10u;
    }
    if (q <= 9u) { /* 5^q may divide at most one of the three */
      if (mv % 5u == 0u) vr_tz = f32_mult_of_pow5(mv, q);
      else if (accept) vm_tz = f32_mult_of_pow5(mm, q);
      else vp -= f32_mult_of_pow5(mp, q) ? 1u : 0u;
    }
  } else {
    const u32 q = f32_log10_pow5((u32)-e2);
    e10 = (int)q + e2;
    const u32 i = (u32)(-e2) - q;
    const int k = (int)kF32Text.bits[i] - 61;
    u32 j = (u32)((int)q - k);
    vr = f32_mul_shift(mv, kF32Text.pow5[i], j);
    vp = f32_mul_shift(mp, kF32Text.pow5[i], j);
    vm = f32_mul_shift(mm, kF32Text.pow5[i], j);
    if (q != 0u && (vp - 1u) / 10u <= vm / 10u) {
      j = (u32)((int)q - 1 - ((int)kF32Text.bits[i + 1u] - 61));
      last = f32_mul_shift(mv, kF32Text.pow5[i + 1u], j) % 10u;
    }
    if (q <= 1u) { /* mv = 4 m2 is a multiple of 2^q; mm of 2 exactly when mm_shift, mp never */
      vr_tz = true;
      if (accept) vm_tz = mm_shift == 1u;
      else vp--;
    } else if (q < 31u) {
      vr_tz = (mv & ((1u << (q - 1u)) - 1u)) == 0u;
    }
  }
  u32 removed = 0, out;
  if (vm_tz || vr_tz) { /* rare: exact halves and bounds that are themselves short */
    while (vp / 10u > vm / 10u) {
      vm_tz = vm_tz && vm % 10u == 0u;
      vr_tz = vr_tz && last == 0u;
      last = vr % 10u;
      vr /= 10u, vp /= 10u, vm /= 10u;
      removed++;
    }
    if (vm_tz)
      while (vm % 10u == 0u) {
        vr_tz = vr_tz && last == 0u;
        last = vr % 10u;
        vr /= 10u, vp /= 10u, vm /= 10u;
        removed++;
      }
    if (vr_tz && last == 5u && vr % 2u == 0u) last = 4u; /* exactly half: to even */
    out = vr + (((vr == vm && (!accept || !vm_tz)) || last >= 5u) ? 1u : 0u);
  } else {
    while (vp / 10u > vm / 10u) {
      last = vr % 10u;
      vr /= 10u, vp /= 10u, vm /= 10u;
      removed++;
    }
    out = vr + ((vr == vm || last >= 5u) ? 1u : 0u);
  }
  *digits = out;
  *exp10 = e10 + (int)removed;
}

/* the digits of v in `width` columns, zeros in front (v < 10^width <= 10^9) */
template <typename S>
__device__ __forceinline__ void f32_text_padded(S& s, u32 v, u32 width) {
  u32 nd = 1;
  while (nd < 9u && v >= kF32Text.pow10[nd]) nd++;
  for (u32 k = nd; k < width; k++) s.c((u8)'0');
  s.dec((u64)v);
}

/* The text of the f32 with this bit pattern, at most 16 bytes.  With `len` digits, k = the exponent of the last and
 * kk = len + k = the place of the decimal point (pretty::format32):
 *   0 <= k && kk <= 13 : digits, k zeros, ".0"         0 < kk <= 13 : dddd.ddd
 *   -6 < kk <= 0       : "0.", -kk zeros, digits       else         : d[.ddd]e<kk - 1> */
template <typename S>
__device__ __forceinline__ void f32_text_emit(S& s, u32 bits) {
  const u32 mant = bits & 0x7FFFFFu, expo = (bits >> 23) & 0xFFu;
  const bool neg = (bits >> 31) != 0u;
  if (expo == 0xFFu && mant != 0u) {
    s.c((u8)'N'), s.c((u8)'a'), s.c((u8)'N');
    return;
  }
  if (neg) s.c((u8)'-');
  if (expo == 0xFFu) {
    s.c((u8)'i'), s.c((u8)'n'), s.c((u8)'f');
    return;
  }
  if (expo == 0u && mant == 0u) {
    s.c((u8)'0'), s.c((u8)'.'), s.c((u8)'0');
    return;
  }
  u32 d;
  int k;
  f32_shortest(mant, expo, &d, &k);
  u32 len = 1;
  while (len < 9u && d >= kF32Text.pow10[len]) len++;
  const int kk = (int)len + k;
  if (0 <= k && kk <= 13) {
    s.dec((u64)d);
    for (int z = 0; z < k; z++) s.c((u8)'0');
    s.c((u8)'.'), s.c((u8)'0');
  } else if (0 < kk && kk <= 13) {
    const u32 f = (u32)-k, p = kF32Text.pow10[f]; /* 0 < f < len */
    s.dec((u64)(d / p));
    s.c((u8)'.');
    f32_text_padded(s, d % p, f);
  } else if (-6 < kk && kk <= 0) {
    s.c((u8)'0'), s.c((u8)'.');
    for (int z = 0; z < -kk; z++) s.c((u8)'0');
    s.dec((u64)d);
  } else {
    const u32 p = kF32Text.pow10[len - 1u];
    s.c((u8)('0' + d / p));
    if (len > 1u) {
      s.c((u8)'.');
      f32_text_padded(s, d % p, len - 1u);
    }
    s.c((u8)'e');
    const int e = kk - 1;
    if (e < 0) s.c((u8)'-');
    s.dec((u64)(e < 0 ? -e : e));
  }
}

#endif /* WGA_F32_TEXT_H */
