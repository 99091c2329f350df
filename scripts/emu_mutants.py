#!/usr/bin/env python3
"""Mutation check of the kernels against the emulator suite: the op walks' 32-bit corners (--table walks, the default) and the
file readers, the `.gz` writer and the MAF walks' long blocks (--table readers: K13, K14, K15, K18, K3 / K4).  CPU ONLY: it builds the SIMT-emulator library and runs
tests/test_emu_parity.py on it; it is not part of pytest and is never run on a GPU machine.

Each row of a table makes one kernel subtly wrong (one exact text edit in wgatools_amd/csrc).  The script copies the tree to a
temporary directory, and for every row applies the edit there, rebuilds tests/emu/libwgaemu.so (build.build_emu(force=True)),
runs `pytest tests/test_emu_parity.py -k <the row's expression>` in one process and prints KILLED (a test failed) or SURVIVED
(all passed).  A first row without an edit must PASS: a suite that fails on the right kernels kills nothing.  Nothing outside
the temporary copy is touched.

    python scripts/emu_mutants.py                  # the working tree's tests
    python scripts/emu_mutants.py --tests-rev REV  # tests/parity_cases.py and tests/test_emu_parity.py as of commit REV
    python scripts/emu_mutants.py --only k5_hi k7_nxt
    python scripts/emu_mutants.py --table readers  # MUTANTS_READERS instead of MUTANTS

profiles/emu_mutants.txt holds both outputs for the commit that added the wide-step cases, profiles/emu_mutants_readers.txt
those of the readers' table for the commit that added it.
"""
import argparse
import os
import re
import shutil
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = "wgatools_amd/csrc/"
TEST_FILES = ("tests/parity_cases.py", "tests/test_emu_parity.py")

# name, file, exact old text (must occur exactly once), new text, pytest -k
MUTANTS = [
    ("k12_scan", CSRC + "wga_k12_dotplot.h",
     "const u32 rl = wave_incl_scan_u32(sr & 0xFFFFu), rh = wave_incl_scan_u32(sr >> 16);",
     "const u32 rl = wave_incl_scan_u32(sr), rh = 0;", "dotplot"),
    ("k7_scan", CSRC + "wga_k7_paf_call.h",
     "tl = wave_incl_scan_u32(tsum & 0xFFFFu), th = wave_incl_scan_u32(tsum >> 16);",
     "tl = wave_incl_scan_u32(tsum), th = 0;", "paf_call"),
    ("k1_wide", CSRC + "wga_k1_stat.h",
     "if (__ballot(s_t >= (1u << 26)) == 0ull) { /* wave-uniform */",
     "if (true) {", "stat"),
    ("kclass_wide", CSRC + "wga_k_class.h",
     "if (__ballot(p[4] >= (1u << 26)) == 0ull) { /* wave-uniform */",
     "if (true) {", "pafpseudo or class_sums"),
    ("k5_hi", CSRC + "wga_k5_pafcov.h",
     "return wave_sum_u32_wide((u32)p) + (wave_sum_u32_wide((u32)(p >> 32)) << 32);",
     "return wave_sum_u32_wide((u32)p);", "pafcov"),
    ("k7_nxt", CSRC + "wga_k7_paf_call.h",
     "if (lane == 63u) nxt = k0 + 256u < nops ? (rec[k0 + 256u] & 15u) : 0xFu;",
     "if (lane == 63u) nxt = 0xFu;", "paf_call"),
    ("k12_cut", CSRC + "wga_k12_dotplot.h",
     "brk[e] = (isi[e] || isd) && (u64)len[e] > cutoff;",
     "brk[e] = (isi[e] || isd) && len[e] > (u32)cutoff;", "dotplot"),
    # controls: the suite caught these before the wide-step cases came
    ("control_k10", CSRC + "wga_k10_chain.h",
     "+ wave_sum_u32_wide(tl) > 0xFFFFFFFFull) return 2;",
     "+ wave_sum_u32_wide(tl) > ~0ull) return 2;", "chain"),
    ("control_k7_carry", CSRC + "wga_k7_paf_call.h",
     "if (lane == 0) prev = carry_code;",
     "if (lane == 0) prev = 0xFu;", "paf_call"),
    ("control_dec32", CSRC + "wga_text_out.h",
     "if (v < 0x100000000ull) {",
     "if (true) {", "chain"),
    ("control_k7_sv", CSRC + "wga_k7_paf_call.h",
     "(u64)len[e] > svlen || cont_follows",
     "len[e] > (u32)svlen || cont_follows", "paf_call"),
]

# The readers, the .gz writer and the long blocks of the MAF walks.  The K3 rows select `test_maf_ and not split`: `maf` alone
# would take every paf2maf test along.
K13, K15, K18, K3 = CSRC + "wga_k13_splitters.h", CSRC + "wga_k15_fasta.h", CSRC + "wga_k18_bgzf_deflate.h", CSRC + "wga_k3_maf.h"
MAF_WALKS = "test_maf_ and not split"
MUTANTS_READERS = [
    ("k13_emptycg", K13, "if (fe - fs >= 5u && text[fs] == (u8)'c'", "if (fe - fs > 5u && text[fs] == (u8)'c'", "paf_split"),
    ("k13_digits20", K13, "if (a >= b || b - a > 20u) return false;", "if (a >= b || b - a > 19u) return false;", "paf_split or maf_split"),
    ("k15_lonecr", K15, "const bool eol = ch == (u8)'\\n' || (ch == (u8)'\\r' && nx == (u8)'\\n');",
     "const bool eol = ch == (u8)'\\n' || ch == (u8)'\\r';", "fasta_pool"),
    ("k15_hdr_gt", K15, "hm |= (ch == (u8)'>' && prev == (u8)'\\n') ? 1u << j : 0u;",
     "hm |= (ch == (u8)'>' && (prev == (u8)'\\n' || prev == (u8)'\\r')) ? 1u << j : 0u;", "fasta_pool"),
    ("k18_halve", K18, "if (s <= 256u && s_wt[s]) s_wt[s] = (s_wt[s] + 1u) >> 1;", "if (s <= 256u && s_wt[s]) s_wt[s] = 1u;", "bgzf_deflate"),
    ("k18_rank", K18, "const u32 wv = s <= 256u ? s_wt[s] : 0u;", "const u32 wv = s <= 256u && s_wt[s] ? 1u + (s_wt[s] >> 3) : 0u;",
     "bgzf_deflate"),
    ("k18_tie", K18, "if (la <= nq) {", "if (la < nq) {", "bgzf_deflate"),
    ("k3_short_max", K3, "#define WGA_MAF_SHORT_MAX 61440u", "#define WGA_MAF_SHORT_MAX 80000u", MAF_WALKS),
    ("k3_fold", K3, "if (++since == WGA_MAF_FOLD_STEPS) {", "if (++since == 40u) {", MAF_WALKS),
    ("k3_tail_lane", K3, "const u32 vidx = !in ? 32u : tail ? 32u - rem : 0u;", "const u32 vidx = !in ? 32u : tail ? 33u - rem : 0u;", MAF_WALKS),
    ("k3_textpath", K3, "if (__ballot((hi & 0x80808080u) != 0u) == 0ull) { /* wave-uniform; text:", "if (true) { /* wave-uniform; text:",
     MAF_WALKS),
    ("scan_final", CSRC + "wga_scan.h", "u64 ex = block_excl_scan_u64(v, s_w, &tot) + partial[blockIdx.x];",
     "u64 ex = block_excl_scan_u64(v, s_w, &tot);", "fasta_pool or scan_and_scatter"),
    ("txt_digits10", CSRC + "wga_text_out.h", "if (w >= 10000u) return n + 4u;", "if (w >= 10000u) return n + 3u;", MAF_WALKS),
    # rows chosen after reading the kernels
    ("k13_plus", K13, "if (a < b && text[a] == (u8)'+') a++;", "if (false) a++;", "paf_split or maf_split"),
    ("k14_token1", K13, "if (p > prev) { /* a token */", "if (p > prev + 1u) { /* a token */", "maf_split"),
    ("k15_finish", K15, "if (contigs[k].hdr_end + 1u >= n_bytes) contigs[k].pool_off = total;",
     "if (contigs[k].hdr_end + 1u > n_bytes) contigs[k].pool_off = total;", "fasta_pool"),
    ("k15_block_hdr", K15, "while (k + 1 < (i64)nh && contigs[k + 1].hdr_start < c) k++;",
     "while (k + 1 < (i64)nh && contigs[k + 1].hdr_start <= c) k++;", "fasta_pool"),
    ("k18_stored", K18, "const bool stored = dyn >= sto;", "const bool stored = dyn > sto;", "bgzf_deflate"),
    ("k18_depth16", K18, "const bool too_deep = __ballot(deepest > 15u) != 0ull;", "const bool too_deep = __ballot(deepest > 16u) != 0ull;",
     "bgzf_deflate"),
    ("k18_eob", K18, "      c = 1u;\n", "      c = 2u;\n", "bgzf_deflate"),
]
TABLES = {"walks": MUTANTS, "readers": MUTANTS_READERS}


def copy_sources(work):
    """the files git tracks, and the new ones it does not ignore, as they stand in the working tree: no build product travels"""
    names = subprocess.run(["git", "-C", ROOT, "ls-files", "-z", "--cached", "--others", "--exclude-standard"], check=True,
                           stdout=subprocess.PIPE).stdout.decode().split("\0")
    for name in filter(None, names):
        src, dst = os.path.join(ROOT, name), os.path.join(work, name)
        if os.path.isfile(src):                  # a tracked file that was deleted is not there
            os.makedirs(os.path.dirname(dst), exist_ok=True)
            shutil.copy2(src, dst, follow_symlinks=False)


def run(cmd, cwd):
    env = dict(os.environ, WGA_TEST_PROCS="1", PYTHONDONTWRITEBYTECODE="1")
    return subprocess.run(cmd, cwd=cwd, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)


def judge(work, expr):
    """(verdict of the run, pytest's last line) on the tree in `work` as it stands"""
    r = run([sys.executable, "-c", "from wgatools_amd import build; build.build_emu(force=True)"], work)
    if r.returncode:
        return "BUILD FAILED", r.stdout.strip().splitlines()[-1:]
    r = run([sys.executable, "-m", "pytest", "tests/test_emu_parity.py", "-q", "-x", "-p", "no:cacheprovider", "-k", expr], work)
    tail = (r.stdout.strip().splitlines() or [""])[-1]
    failed = [ln.split(" ")[1].split("::")[-1] for ln in r.stdout.splitlines() if ln.startswith("FAILED ")]
    if r.returncode == 0:
        return "passed", tail
    if r.returncode == 1:
        return "failed", "%s  [%s]" % (tail, ", ".join(failed))
    return "ERROR (pytest exit %d)" % r.returncode, tail


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--tests-rev", help="take %s and %s from this commit" % TEST_FILES)
    ap.add_argument("--only", nargs="*", help="names of the rows to run")
    ap.add_argument("--table", choices=sorted(TABLES), default="walks", help="the table of mutants (default: walks)")
    a = ap.parse_args()
    tmp = tempfile.mkdtemp(prefix="emu_mutants_")
    work = os.path.join(tmp, "tree")
    bad = 0
    try:
        copy_sources(work)
        if a.tests_rev:
            for f in TEST_FILES:
                text = subprocess.run(["git", "-C", ROOT, "show", "%s:%s" % (a.tests_rev, f)], check=True,
                                      stdout=subprocess.PIPE).stdout
                with open(os.path.join(work, f), "wb") as fh:
                    fh.write(text)
        print("# tests: %s, table: %s" % (a.tests_rev or "working tree", a.table))
        rows = [m for m in TABLES[a.table] if not a.only or m[0] in a.only]
        exprs = sorted({m[4] for m in rows})
        t0 = time.time()
        verdict, tail = judge(work, " or ".join("(%s)" % e for e in exprs))
        print("%-18s %-10s %s" % ("unmodified", "PASS" if verdict == "passed" else verdict.upper(), tail))
        if verdict != "passed":
            return 2
        for name, path, old, new, expr in rows:
            full = os.path.join(work, path)
            with open(full) as fh:
                src = fh.read()
            assert src.count(old) == 1, "%s: the old text occurs %d times in %s" % (name, src.count(old), path)
            with open(full, "w") as fh:
                fh.write(src.replace(old, new))
            try:
                verdict, tail = judge(work, expr)
            finally:
                with open(full, "w") as fh:
                    fh.write(src)
            word = {"failed": "KILLED", "passed": "SURVIVED"}.get(verdict, verdict)
            bad += word != "KILLED"
            print("%-18s %-10s -k %-26r %s" % (name, word, expr, re.sub(r"=+", "", tail).strip()), flush=True)
        print("# %d of %d not killed, %.0f s" % (bad, len(rows), time.time() - t0))
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
