#!/usr/bin/env python3
"""K34's f64 formatter against the host's format_f64, over three sets of doubles.  CPU only: never run on a GPU machine.

Builds a small stand-alone program (its own main) from wgatools_amd/csrc/wga_f64_text.h — the formatter's source as the kernels
compile it — and wgatools_amd/host/wga_host.cpp (format_f64, over std::to_chars), runs the comparison across threads and writes
the report to profiles/k34_f64_sweep.txt: the sets' sizes and seeds, the first mismatches as bits and both texts, their count
(must be 0) and the longest text (must be <= 24):
  edges    every exponent field x {the 2 048 lowest mantissas, the 2 048 highest, 4 096 seeded random ones}
  random   10^9 seeded random bit patterns (splitmix64 of seed + index: the same set whatever the thread count)
  ratios   (double)a / (double)b for every 0 <= a <= 4 096, 1 <= b <= 4 096

  python3 scripts/f64_text_sweep.py [--threads N] [--random N] [--sanitize]
A run with --sanitize (address + undefined, a reduced --random) or with another --random prints its report and appends it to
the file only with --note.
"""
import argparse
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

MAIN = r"""
#include <atomic>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>
#include <thread>
#include <vector>
typedef unsigned int u32;
typedef unsigned long long u64;
typedef unsigned char u8;
#define __device__
#define __forceinline__ inline
#include "wga_f64_text.h"
#include "wga_host.hpp"

struct Put { /* the sink: bytes into a buffer with room to show an overrun */
  u8 b[48];
  u32 n = 0;
  void c(u8 ch) { if (n < sizeof b) b[n++] = ch; }
  void dec(u64 v) {
    char t[24];
    int k = snprintf(t, sizeof t, "%llu", v);
    for (int i = 0; i < k; i++) c((u8)t[i]);
  }
};
static u64 splitmix(u64 x) {
  x += 0x9E3779B97F4A7C15ull;
  x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
  x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
  return x ^ (x >> 31);
}
static const u64 kMant = (1ull << 52) - 1u;
static u64 seed_edges, seed_random;
/* element x of set `set` */
static u64 pattern(int set, u64 x) {
  if (set == 0) { /* x = exponent field * 8192 + slot */
    const u64 e = x >> 13, s = x & 8191u;
    const u64 m = s < 2048u ? s : s < 4096u ? kMant - (s - 2048u) : splitmix(seed_edges + x) & kMant;
    return e << 52 | m;
  }
  if (set == 1) return splitmix(seed_random + x);
  const double v = (double)(x / 4096u) / (double)(x % 4096u + 1u); /* a = x / 4096 (0 .. 4096), b = x % 4096 + 1 */
  u64 b;
  memcpy(&b, &v, 8);
  return b;
}

int main(int argc, char** argv) {
  const unsigned nthr = (unsigned)atoi(argv[1]);
  const u64 n_random = strtoull(argv[2], nullptr, 0);
  seed_edges = strtoull(argv[3], nullptr, 0), seed_random = strtoull(argv[4], nullptr, 0);
  const u64 sizes[3] = {2048ull * 8192u, n_random, 4097ull * 4096u};
  const char* const names[3] = {"edges ", "random", "ratios"};
  std::atomic<u64> bad{0};
  std::atomic<u32> longest{0};
  std::mutex mu;
  std::vector<std::string> first;
  for (int set = 0; set < 3; set++) {
    std::atomic<u64> next{0};
    const u64 total = sizes[set], step = 1u << 18;
    std::vector<std::thread> pool;
    for (unsigned t = 0; t < nthr; t++)
      pool.emplace_back([&] {
        for (;;) {
          const u64 lo = next.fetch_add(step);
          if (lo >= total) return;
          u32 mylong = 0;
          for (u64 x = lo; x < lo + step && x < total; x++) {
            const u64 bits = pattern(set, x);
            double f;
            memcpy(&f, &bits, 8);
            Put p;
            f64_text_emit(p, bits);
            const std::string want = wga::format_f64(f);
            if (p.n > mylong) mylong = p.n;
            if (want.size() != p.n || memcmp(want.data(), p.b, p.n) != 0) {
              bad++;
              std::lock_guard<std::mutex> g(mu);
              if (first.size() < 20) {
                char line[200];
                snprintf(line, sizeof line, "%s %016llx  kernel source: %.*s  format_f64: %s", names[set], bits, (int)p.n,
                         (const char*)p.b, want.c_str());
                first.push_back(line);
              }
            }
          }
          u32 cur = longest.load();
          while (mylong > cur && !longest.compare_exchange_weak(cur, mylong)) {}
        }
      });
    for (auto& th : pool) th.join();
    printf("%s: %llu doubles compared, mismatches so far: %llu\n", names[set], total, (u64)bad.load());
  }
  for (const auto& l : first) printf("%s\n", l.c_str());
  printf("seeds: edges %llu, random %llu\nmismatches: %llu\nlongest text: %u bytes\n", seed_edges, seed_random, (u64)bad.load(),
         longest.load());
  return bad.load() == 0 && longest.load() <= 24u ? 0 : 1;
}
"""


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--random", default=str(10 ** 9), help="the number of random patterns")
    ap.add_argument("--seeds", default="20261021,34", help="the seeds of the edges' random mantissas and of the random patterns")
    ap.add_argument("--sanitize", action="store_true", help="build with -fsanitize=address,undefined")
    ap.add_argument("--note", action="store_true", help="append this run's report to the file (a reduced or sanitized run)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "k34_f64_sweep.txt"))
    a = ap.parse_args()
    seeds = a.seeds.split(",")
    with tempfile.TemporaryDirectory() as tmp:
        src = os.path.join(tmp, "f64_text_sweep.cpp")
        exe = os.path.join(tmp, "f64_text_sweep")
        with open(src, "w") as f:
            f.write(MAIN)
        cmd = ["g++", "-O2", "-std=c++17", "-Wall", "-I" + os.path.join(ROOT, "wgatools_amd", "csrc"),
               "-I" + os.path.join(ROOT, "wgatools_amd", "host"), src, os.path.join(ROOT, "wgatools_amd", "host", "wga_host.cpp"),
               "-o", exe, "-lz", "-lpthread"]
        if a.sanitize:
            cmd[1:1] = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-g"]
        subprocess.run(cmd, check=True)
        r = subprocess.run([exe, str(a.threads), a.random, seeds[0], seeds[1]], stdout=subprocess.PIPE, text=True)
    head = ("K34's f64 text (wga_f64_text.h, compiled for the host) against format_f64 (wga_host.cpp, std::to_chars)\n"
            "scripts/f64_text_sweep.py%s --random %s, %d threads\n\n" % (" --sanitize" if a.sanitize else "", a.random, a.threads))
    sys.stdout.write(head + r.stdout)
    full = int(a.random, 0) == 10 ** 9 and not a.sanitize
    if full or a.note:
        with open(a.out, "w" if full else "a") as f:
            f.write(("" if full else "\n") + head + r.stdout)
    return r.returncode


if __name__ == "__main__":
    sys.exit(main())
