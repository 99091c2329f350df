#!/usr/bin/env python3
"""The power-of-five tables of wgatools_amd/csrc/wga_f64_text.h, from Python integers.  CPU only.

With bits(x) the bit length of x (Adams, "Ryu", PLDI 2018, section 3.2.1: one 128-bit factor per power):
  kF64Pow5[i]    = 5^i scaled to 125 bits: 5^i >> (bits(5^i) - 125), or << (125 - bits(5^i))            0 <= i < 326
  kF64Pow5Inv[q] = floor(2^(bits(5^q) - 1 + 125) / 5^q) + 1                                              0 <= q < 292
each written as {low 64 bits, high 64 bits}.  326: the largest i is 1076 - (floor(1076 log10 5) - 1) = 325 (a subnormal's
e2 = -1076); 292: the largest q is floor(969 log10 2) - 1 = 290 (e2 = 969 for the largest exponent field), one more is kept.

  python3 scripts/make_f64_text_tables.py            check: the header's literals are these numbers (exit status 1 if not)
  python3 scripts/make_f64_text_tables.py --write    rewrite the block between the header's two marker lines
"""
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "wgatools_amd", "csrc", "wga_f64_text.h")
BEGIN = "/* ---- tables: scripts/make_f64_text_tables.py --write (do not edit by hand) ---- */"
END = "/* ---- end of the generated tables ---- */"
N_POW5, N_POW5_INV, BITCOUNT = 326, 292, 125
M64 = (1 << 64) - 1


def pow5(i):
    p = 5 ** i
    b = p.bit_length()
    return p >> (b - BITCOUNT) if b >= BITCOUNT else p << (BITCOUNT - b)


def pow5_inv(q):
    p = 5 ** q
    return (1 << (p.bit_length() - 1 + BITCOUNT)) // p + 1


def tables():
    """(pow5, pow5_inv): lists of (low, high)"""
    split = lambda v: (v & M64, v >> 64)
    a, b = [split(pow5(i)) for i in range(N_POW5)], [split(pow5_inv(q)) for q in range(N_POW5_INV)]
    assert all(hi < (1 << 61) for _, hi in a) and all(hi <= (1 << 61) for _, hi in b)
    return a, b


def block():
    a, b = tables()
    out = [BEGIN]
    for name, n, rows in (("kF64Pow5", N_POW5, a), ("kF64Pow5Inv", N_POW5_INV, b)):
        out.append("static constexpr u64 %s[%d][2] = {" % (name, n))
        for k in range(0, n, 2):
            out.append("    " + " ".join("{0x%016Xull, 0x%016Xull}," % r for r in rows[k:k + 2]))
        out.append("};")
    out.append(END)
    return "\n".join(out)


def parse(text):
    """the two tables as the header holds them: lists of (low, high)"""
    got = []
    for name in ("kF64Pow5", "kF64Pow5Inv"):
        m = re.search(r"static constexpr u64 %s\[(\d+)\]\[2\] = \{(.*?)\n\};" % name, text, re.S)
        rows = [(int(lo, 16), int(hi, 16)) for lo, hi in re.findall(r"\{0x([0-9A-F]{16})ull, 0x([0-9A-F]{16})ull\}", m.group(2))]
        assert len(rows) == int(m.group(1)), name
        got.append(rows)
    return got


def main():
    text = open(HEADER).read()
    lo, hi = text.index(BEGIN), text.index(END) + len(END)
    if "--write" in sys.argv[1:]:
        with open(HEADER, "w") as f:
            f.write(text[:lo] + block() + text[hi:])
        return 0
    a, b = tables()
    ga, gb = parse(text)
    bad = [("kF64Pow5", i) for i in range(N_POW5) if i >= len(ga) or ga[i] != a[i]]
    bad += [("kF64Pow5Inv", q) for q in range(N_POW5_INV) if q >= len(gb) or gb[q] != b[q]]
    print("%d + %d entries, %d differ%s" % (len(ga), len(gb), len(bad), (": %r" % bad[:8]) if bad else ""))
    return 1 if bad or len(ga) != N_POW5 or len(gb) != N_POW5_INV else 0


if __name__ == "__main__":
    sys.exit(main())
