#!/usr/bin/env python3
"""K33's f32 formatter against the host's format_f32, for ALL 2^32 bit patterns.  CPU only: never run on a GPU machine.

Builds a small stand-alone program (its own main) from wgatools_amd/csrc/wga_f32_text.h — the formatter's source as the kernels
compile it — and wgatools_amd/host/wga_host.cpp (format_f32, over std::to_chars), runs the comparison across threads and writes
the report to profiles/k33_f32_exhaustive.txt: the first mismatches, their count (must be 0) and the longest text (must be <= 16).

  python3 scripts/f32_text_exhaustive.py [--threads N] [--sanitize]
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
#include "wga_f32_text.h"
#include "wga_host.hpp"

struct Put { /* the sink: bytes into a buffer with room to show an overrun */
  u8 b[40];
  u32 n = 0;
  void c(u8 ch) { if (n < sizeof b) b[n++] = ch; }
  void dec(u64 v) {
    char t[24];
    int k = snprintf(t, sizeof t, "%llu", v);
    for (int i = 0; i < k; i++) c((u8)t[i]);
  }
};

int main(int argc, char** argv) {
  const unsigned nthr = argc > 1 ? (unsigned)atoi(argv[1]) : 8u;
  const u64 total = argc > 2 ? strtoull(argv[2], nullptr, 0) : (1ull << 32);
  std::atomic<u64> next{0}, bad{0};
  std::atomic<u32> longest{0};
  std::mutex mu;
  std::vector<std::string> first;
  const u64 step = 1u << 20;
  std::vector<std::thread> pool;
  for (unsigned t = 0; t < nthr; t++)
    pool.emplace_back([&] {
      for (;;) {
        const u64 lo = next.fetch_add(step);
        if (lo >= total) return;
        u32 mylong = 0;
        for (u64 x = lo; x < lo + step && x < total; x++) {
          const u32 bits = (u32)x;
          float f;
          memcpy(&f, &bits, 4);
          Put p;
          f32_text_emit(p, bits);
          const std::string want = wga::format_f32(f);
          if (p.n > mylong) mylong = p.n;
          if (want.size() != p.n || memcmp(want.data(), p.b, p.n) != 0) {
            bad++;
            std::lock_guard<std::mutex> g(mu);
            if (first.size() < 20) {
              char line[160];
              snprintf(line, sizeof line, "%08x  kernel source: %.*s  format_f32: %s", bits, (int)p.n, (const char*)p.b, want.c_str());
              first.push_back(line);
            }
          }
        }
        u32 cur = longest.load();
        while (mylong > cur && !longest.compare_exchange_weak(cur, mylong)) {}
      }
    });
  for (auto& th : pool) th.join();
  for (const auto& l : first) printf("%s\n", l.c_str());
  printf("patterns compared: %llu\nmismatches: %llu\nlongest text: %u bytes\n", total, (u64)bad.load(), longest.load());
  return bad.load() == 0 && longest.load() <= 16u ? 0 : 1;
}
"""


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--threads", type=int, default=min(os.cpu_count() or 8, 64))
    ap.add_argument("--patterns", default=str(1 << 32), help="compare only the first N patterns (a quick look)")
    ap.add_argument("--sanitize", action="store_true", help="build with -fsanitize=address,undefined")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "k33_f32_exhaustive.txt"))
    a = ap.parse_args()
    with tempfile.TemporaryDirectory() as tmp:
        src = os.path.join(tmp, "f32_text_exhaustive.cpp")
        exe = os.path.join(tmp, "f32_text_exhaustive")
        with open(src, "w") as f:
            f.write(MAIN)
        cmd = ["g++", "-O2", "-std=c++17", "-Wall", "-I" + os.path.join(ROOT, "wgatools_amd", "csrc"),
               "-I" + os.path.join(ROOT, "wgatools_amd", "host"), src, os.path.join(ROOT, "wgatools_amd", "host", "wga_host.cpp"),
               "-o", exe, "-lz", "-lpthread"]
        if a.sanitize:
            cmd[1:1] = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-g"]
        subprocess.run(cmd, check=True)
        r = subprocess.run([exe, str(a.threads), a.patterns], stdout=subprocess.PIPE, text=True)
    head = ("K33's f32 text (wga_f32_text.h, compiled for the host) against format_f32 (wga_host.cpp, std::to_chars)\n"
            "scripts/f32_text_exhaustive.py%s, %d threads\n\n" % (" --sanitize" if a.sanitize else "", a.threads))
    sys.stdout.write(head + r.stdout)
    if int(a.patterns, 0) == 1 << 32 and not a.sanitize:
        with open(a.out, "w") as f:
            f.write(head + r.stdout)
    return r.returncode


if __name__ == "__main__":
    sys.exit(main())
