#!/usr/bin/env python3
"""gpu_record_rows_count_ab.py PARENT_LIB BRANCH_LIB [OUT] — the count call of wga_stat_rows (K33) and of wga_dotplot_overview (K34)
under two builds of libwgahip.so.

The count call is the plan kernel, the scan of the plan and one 8-byte copy back (the pattern of time_two_calls in
scripts/gpu_stat_rows_e2e.py: host clock, the call synchronises through its copy).  Rows: 160 014 and 347 197, the row counts of
that script's two shapes; names of a few letters, numbers of up to 9 digits.  One repetition is a fresh child process on one
library: per entry and shape a warm-up, then the median of INNER calls in a row.  The children alternate between the libraries,
REPS each.  (Two engines in ONE process do not compare: the one created second was 1 to 3 % ahead whichever library it had.)
The yardstick is PARENT_LIB: the median of the branch's repetitions must lie inside the min-max spread of the parent's.  Both
series go to OUT (default: stdout only).  Exit status 1 when a median lies ABOVE the parent's spread."""
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np

ROWS = (160014, 347197)
ENTRIES = ("wga_stat_rows", "wga_dotplot_overview")
REPS, INNER = 7, 20


def arrays(engine, n):
    rnd = np.random.default_rng(3300 + n)
    names = b"".join(b"chr%d" % k for k in range(1, 25)) + b"".join(b"q%d" % k for k in range(40))
    at = np.cumsum([0] + [len(b"chr%d" % k) for k in range(1, 25)] + [len(b"q%d" % k) for k in range(40)])
    t, q = rnd.integers(0, 24, n), rnd.integers(24, 64, n)
    cnt = np.zeros(n, dtype=engine.COUNTS_DTYPE)
    for f in cnt.dtype.names:
        cnt[f] = rnd.integers(0, 40, n)
    cnt["match"] = rnd.integers(100, 10 ** 6, n)
    heads = {}
    for dt in (engine.STAT_ROW_HEAD_DTYPE, engine.DOTPLOT_OV_HEAD_DTYPE):
        h = np.zeros(n, dtype=dt)
        for f in dt.names:
            if not f.endswith(("_off", "_len")):
                h[f] = rnd.integers(1, 10 ** 9, n)
        h["rname_off"], h["rname_len"] = at[t], at[t + 1] - at[t]
        h["qname_off"], h["qname_len"] = at[q], at[q + 1] - at[q]
        heads[dt] = h
    return names, heads, cnt


def count(eng, engine, entry, n, n_name_bytes, d):
    tot = C.c_uint64(0)
    if entry == "wga_stat_rows":
        rc = eng.lib.wga_stat_rows(eng.ctx, n, d["names"].ptr, n_name_bytes, d[engine.STAT_ROW_HEAD_DTYPE].ptr, d["cnt"].ptr,
                                   d["work"].ptr, d["row_off"].ptr, C.byref(tot), None)
    else:
        rc = eng.lib.wga_dotplot_overview(eng.ctx, n, d["names"].ptr, n_name_bytes, d[engine.DOTPLOT_OV_HEAD_DTYPE].ptr, d["cnt"].ptr, 0,
                                          d["work"].ptr, d["row_off"].ptr, C.byref(tot), None)
    eng._check(rc)
    return int(tot.value)


def child(path):
    """one repetition of every entry and shape on the library `path`: a JSON list of [entry, rows, ms, total_bytes]"""
    import torch  # noqa: F401  (loads the HIP runtime the engine shares)
    from wgatools_amd import _lib, engine
    eng = engine.Engine(0, _lib.load(path))
    out = []
    for n in ROWS:
        names, heads, cnt = arrays(engine, n)
        d = {dt: eng.upload(h) for dt, h in heads.items()}
        d.update(names=eng.upload(np.frombuffer(names + b"\0" * 16, dtype=np.uint8)), cnt=eng.upload(cnt),
                 work=eng.empty(int(eng.lib.wga_stat_rows_work_bytes(n)), np.uint8), row_off=eng.empty(n + 1, np.uint64))
        for entry in ENTRIES:
            t = []
            for k in range(2 * INNER):                                            # the first INNER warm up
                eng.sync()
                t0 = time.perf_counter()
                total = count(eng, engine, entry, n, len(names), d)
                t.append(time.perf_counter() - t0)
            out.append([entry, n, statistics.median(t[INNER:]) * 1e3, total])
    eng.close()
    print(json.dumps(out))
    return 0


def main():
    if len(sys.argv) == 3 and sys.argv[1] == "--child":
        return child(sys.argv[2])
    if len(sys.argv) not in (3, 4):
        sys.exit(__doc__)
    libs = {"parent": sys.argv[1], "branch": sys.argv[2]}
    got = {}
    for rep in range(REPS):
        for k, path in libs.items():
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", path], stdout=subprocess.PIPE, text=True, timeout=120)
            if r.returncode != 0:
                sys.exit("the child on %s ended with %d" % (path, r.returncode))
            for entry, n, ms, total in json.loads(r.stdout.strip().split("\n")[-1]):
                got.setdefault((entry, n), {"parent": [], "branch": [], "totals": set()})
                got[(entry, n)][k].append(ms)
                got[(entry, n)]["totals"].add(total)
    lines, slower = ["count call of K33 and K34, ms (host clock), a repetition = a fresh process: a warm-up, then the median of %d "
                     "calls; %d repetitions a library, the libraries alternating" % (INNER, REPS)], False
    for (entry, n), g in got.items():
        assert len(g["totals"]) == 1, g["totals"]                                 # both builds plan the same bytes
        lo, hi, med = min(g["parent"]), max(g["parent"]), statistics.median(g["branch"])
        verdict = "inside" if lo <= med <= hi else "BELOW (faster)" if med < lo else "ABOVE (slower)"
        slower = slower or med > hi
        lines.append("%s, %d rows, %.1f MB of text" % (entry, n, g["totals"].pop() / 1e6))
        for k in libs:
            lines.append("    %-6s %s   median %.4f" % (k, " ".join("%.4f" % v for v in g[k]), statistics.median(g[k])))
        lines.append("    the branch's median %.4f against the parent's spread %.4f .. %.4f: %s" % (med, lo, hi, verdict))
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if len(sys.argv) == 4:
        with open(sys.argv[3], "w") as f:
            f.write(text)
    return 1 if slower else 0


if __name__ == "__main__":
    sys.exit(main())
