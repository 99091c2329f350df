"""`validate --fix` file to file: a synthetic PAF of N records with cg:Z: tags of a mean of 5 000 ops (configs[1]'s records and
ops at the default N: about 2.2 GB of text), one record in ten with a wrong query end and one in ten with a wrong target end,
validated and fixed three ways: this tree (K29, the device path; three runs), this tree with WGA_VALIDATE_WRITER=host (every record parsed and
printed again on the host; one run) and, when WGA_PARENT_CLI names it, the parent commit's `wgatools` binary (five runs); all
under WGA_TIMING=1, one process at a time, each under its own time limit; a step that fails ends the script.  The reports and
the fixed files of the three ways must be equal byte for byte.  Then the fill call alone: both calls of wga_paf_fix on the first
piece of the file in this process, the fill call timed around a synchronise.  Wall times, phase lines and the fill call's bytes
and time go to profiles/r07_validate_fix_e2e.txt.  Without a visible MI355X the file says so and holds no figure.
The rule: the command counts as faster only if the device path's slowest of three runs is below the parent's fastest of five by
more than the parent's spread (slowest - fastest).  What to compare the fill call with: the 5.85 TB/s of a plain copy (bytes
read + bytes written per second).
Usage: python scripts/gpu_validate_fix_e2e.py [N_RECORDS] [WORKDIR]      (default 100 000 records, a temporary directory)"""
import ctypes as C
import filecmp
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "profiles", "r07_validate_fix_e2e.txt")
MEAN_OPS, LIMIT_S = 5000, 600


def write_paf_file(path, n, seed=7):
    """records on 40 queries x 25 targets; every cg:Z: is a run of ops out of one random pool, the ends are the ones the CIGAR
    asks for except where a record is chosen to be wrong.  Returns (wrong query ends, wrong target ends)"""
    rng = np.random.default_rng(seed)
    n_pool = 1 << 22
    lens = rng.integers(1, 2000, n_pool)
    kinds = rng.integers(0, 4, n_pool)                                          # = X I D
    codes = np.frombuffer(b"=XID", dtype=np.uint8)[kinds]
    ops = [b"%d%c" % (a, c) for a, c in zip(lens.tolist(), codes.tolist())]
    off = np.concatenate([[0], np.cumsum([len(o) for o in ops])])
    q_sum = np.concatenate([[0], np.cumsum(np.where(kinds != 3, lens, 0))])     # = X I advance the query
    t_sum = np.concatenate([[0], np.cumsum(np.where(kinds != 2, lens, 0))])     # = X D advance the target
    pool = b"".join(ops)
    n_ops = rng.integers(1, 2 * MEAN_OPS, n)
    first = rng.integers(0, n_pool - 2 * MEAN_OPS, n)
    qs, ts = rng.integers(0, 10 ** 8, n), rng.integers(0, 10 ** 8, n)
    q, t = rng.integers(0, 40, n), rng.integers(0, 25, n)
    q_wrong, t_wrong = rng.random(n) < 0.1, rng.random(n) < 0.1
    delta = rng.integers(1, 10 ** 4, n)
    with open(path, "wb") as f:
        for k in range(n):
            a, z = int(first[k]), int(first[k] + n_ops[k])
            qe = int(qs[k] + q_sum[z] - q_sum[a]) + (int(delta[k]) if q_wrong[k] else 0)
            te = int(ts[k] + t_sum[z] - t_sum[a]) - (int(delta[k]) % 7 + 1 if t_wrong[k] else 0)
            f.write(b"query%d\t200000000\t%d\t%d\t%s\tchr%d\t150000000\t%d\t%d\t%d\t%d\t60\ttp:A:P\tcg:Z:" % (
                q[k], qs[k], qe, b"+-"[k & 1:(k & 1) + 1], t[k], ts[k], te, n_ops[k], 2 * n_ops[k]))
            f.write(pool[int(off[a]):int(off[z])])
            f.write(b"\n")
    return int(q_wrong.sum()), int(t_wrong.sum())


def fill_call(src, report, reps=5):
    """split, plan, tokeniser, K1 and both calls of wga_paf_fix on the first piece (at most 1 GiB, cut at a line end), the fill
    call timed"""
    import torch  # noqa: F401
    from wgatools_amd import build, engine, _lib
    eng = engine.Engine(0, _lib.load(build.HIP_LIB))
    with open(src, "rb") as f:
        data = f.read(1 << 30)
    data = data[:data.rindex(b"\n") + 1]
    d_text = eng.upload(np.frombuffer(data + b"\0" * 16, dtype=np.uint8))
    n = eng.paf_split(d_text, len(data))
    d_lines = eng.empty(n + 1, engine.PAF_LINE_DTYPE)
    eng.paf_split(d_text, len(data), d_lines)
    nr, bad, beg, end = eng.paf_fix_plan(d_text, len(data), d_lines, n)
    if bad is not None or nr == 0:
        report.append("fill call: the first piece is not taken (line %s): no figure" % bad)
        eng.close()
        return
    cnt, err = eng.cigar_tokenise_spans(nr, d_text, beg, end)
    off = eng.exclusive_scan_u64(nr, cnt)
    tot = int(off.numpy()[-1])
    ops = eng.empty(tot + 4, np.uint32)
    eng.cigar_tokenise_spans(nr, d_text, beg, end, op_cnt=cnt, err=err, ops=ops, op_off=off)
    batch = engine.Batch(ops, off, eng.upload(np.zeros(nr + 16, np.uint8)), nr, tot)
    counts, diag, _ = eng.cigar_stat(batch, want_tiles=False)
    work = eng.empty(int(eng.lib.wga_paf_fix_work_bytes(n)), np.uint8)
    sizes = np.zeros(1, dtype=engine.PAF_FIX_SIZES_DTYPE)
    args = (eng.ctx, d_text.ptr, len(data), d_lines.ptr, n, counts.ptr, nr, work.ptr, sizes.ctypes.data)
    eng.sync()
    t0 = time.perf_counter()
    eng._check(eng.lib.wga_paf_fix(*args, None, None, None))
    t_count = time.perf_counter() - t0
    rows_bytes = int(sizes["rows_bytes"][0])
    rows = eng.empty(rows_bytes + 16, np.uint8)
    ql = eng.empty(int(sizes["qlist_bytes"][0]) + 16, np.uint8)
    tl = eng.empty(int(sizes["tlist_bytes"][0]) + 16, np.uint8)
    times = []
    for _ in range(reps + 1):                      # the first one warms up
        eng.sync()
        t0 = time.perf_counter()
        eng._check(eng.lib.wga_paf_fix(*args, rows.ptr, ql.ptr, tl.ptr))
        eng.sync()
        times.append(time.perf_counter() - t0)
    best = min(times[1:])
    report.append("fill call on the first piece: %d lines, %d records, %.1f MB in, %.1f MB of rows, %d + %d bad ends" % (
        n, nr, len(data) / 1e6, rows_bytes / 1e6, int(sizes["n_q_bad"][0]), int(sizes["n_t_bad"][0])))
    report.append("    count call %.3f ms (host clock, synchronises; newline list, record scan, line pass, four scans)" % (t_count * 1e3))
    report.append("    fill call  %.3f ms best of %d (host clock around a synchronise; rows and both lists): %.2f TB/s of rows written, "
                  "%.2f TB/s read + written, next to a plain copy's 5.85 TB/s" % (best * 1e3, reps, rows_bytes / best / 1e12,
                                                                                 2 * rows_bytes / best / 1e12))
    eng.close()


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 100000
    from wgatools_amd import build
    have = False
    if os.path.exists(build.HIP_LIB):
        try:
            import torch  # noqa: F401  first: the library then shares torch's HIP runtime
            have = C.CDLL(build.HIP_LIB).wga_device_count() > 0
        except OSError:
            have = False
    report, ok = [], False
    if not have or not os.path.exists(build.CLI_BIN):
        report.append("no MI355X visible (or wgatools not built): this file holds no figures")
    else:
        work = sys.argv[2] if len(sys.argv) > 2 else tempfile.mkdtemp(prefix="validate_fix_e2e_")
        src = os.path.join(work, "in.paf")
        nq, nt = write_paf_file(src, n)
        report.append("validate --fix file to file: %d records, %.1f MB of PAF, %d wrong query ends, %d wrong target ends" % (
            n, os.path.getsize(src) / 1e6, nq, nt))
        parent = os.environ.get("WGA_PARENT_CLI")
        ways = [("this tree (device path)", build.CLI_BIN, {}, 3), ("this tree, WGA_VALIDATE_WRITER=host", build.CLI_BIN, {"WGA_VALIDATE_WRITER": "host"}, 1)]
        if parent and os.path.exists(parent):
            ways.append(("parent commit's binary", parent, {}, 5))
        else:
            report.append("WGA_PARENT_CLI not set: the parent commit's binary is NOT measured")
        ok = True
        walls, kept = {}, []
        for name, cli, env, runs in ways:
            for k in range(runs):
                rep, fixed = os.path.join(work, "report_%d.txt" % len(kept)), os.path.join(work, "fixed_%d.paf" % len(kept))
                t0 = time.perf_counter()
                r = subprocess.run(["timeout", "-k", "10", str(LIMIT_S), cli, "validate", src, "--fix", fixed, "-o", rep, "-r"],
                                   env=dict(os.environ, WGA_TIMING="1", **env), stdout=subprocess.PIPE, stderr=subprocess.PIPE)
                wall = time.perf_counter() - t0
                walls.setdefault(name, []).append(wall)
                report.append("  %s, run %d: exit %d, wall %.3f s, %.1f MB fixed" % (
                    name, k + 1, r.returncode, wall, os.path.getsize(fixed) / 1e6 if os.path.exists(fixed) else 0.0))
                if k == 0 or r.returncode != 0:
                    report.extend("      " + ln for ln in r.stderr.decode(errors="replace").strip().split("\n"))
                if r.returncode != 0:                  # nothing more is started on the device behind a failed step
                    report.append("step failed: the run ends here")
                    ok = False
                    break
                if k == 0:
                    kept.append((rep, fixed))
                else:                                  # later runs of a way: compared with its first, then dropped
                    same = filecmp.cmp(kept[-1][0], rep, shallow=False) and filecmp.cmp(kept[-1][1], fixed, shallow=False)
                    ok = ok and same
                    os.remove(rep)
                    os.remove(fixed)
            if not ok:
                break
        if ok:
            same = all(filecmp.cmp(kept[0][0], r, shallow=False) and filecmp.cmp(kept[0][1], f, shallow=False) for r, f in kept[1:])
            report.append("reports and fixed files equal over the %d ways: %s" % (len(kept), same))
            ok = same
        for r, f in kept:
            for p in (r, f):
                if os.path.exists(p):
                    os.remove(p)
        dev, par = walls.get("this tree (device path)"), walls.get("parent commit's binary")
        if ok and dev and par and len(par) == 5:
            spread = max(par) - min(par)
            faster = max(dev) < min(par) - spread
            report.append("device path: slowest of three %.3f s; parent: fastest of five %.3f s, spread %.3f s: %s" % (
                max(dev), min(par), spread, "faster" if faster else "NOT shown to be faster"))
        elif ok:
            report.append("no parent runs: nothing is said about faster or slower")
        if ok:
            fill_call(src, report)
        if os.path.exists(src):
            os.remove(src)
    text = "\n".join(report) + "\n"
    with open(OUT, "w") as f:
        f.write(text)
    sys.stdout.write(text)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
