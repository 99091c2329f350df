"""`stat` (the merged table, K36) file to file, after scripts/gpu_stat_rows_e2e.py and with its machinery: `stat -f paf` on the
short-record PAF (1 000 000 records x mean 500 ops) once with the generator's names and once with every record its own pair (the
record's number appended to the query name), and `stat` on configs[2]'s MAF (2 000 000 blocks of 1 500 columns).  Each shape is
run three ways: this tree (the device path) three times, the parent commit's `wgatools` binary five times when WGA_PARENT_CLI
names it, and this tree with WGA_STAT_WRITER=host once.  The parent's spread of wall times is the margin: "faster" needs the device
path's slowest run below the parent's fastest by more than that spread, "slower" is the same rule turned round, and if neither
holds the answer is "not shown".  All under WGA_TIMING=1 (the phase lines name `stat table (device)` or `stat table (host)`), one
process on the GPU at a time, each under its own time limit; the first step that fails ends the script.  The outputs of a shape
must be equal byte for byte.  Then, in a child process on the records of the file's first piece, the three calls of wga_stat_pairs
(the grouping, the sums, a repeat with d_inv_in) and both calls of wga_stat_pair_rows, each timed around a synchronise.
Everything goes to profiles/r07_stat_pairs_e2e.txt.  Without a visible MI355X the file says that it holds no figures.
Usage: python scripts/gpu_stat_pairs_e2e.py [SCALE] [WORKDIR]   (SCALE divides the shapes' record counts, default 1; default a
temporary directory)"""
import ctypes as C
import os
import shutil
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import gpu_maf2paf_e2e as maf_e2e  # noqa: E402
import gpu_stat_rows_e2e as rows_e2e  # noqa: E402
from gpu_maf2paf_e2e import child, probe  # noqa: E402

OUT = os.path.join(ROOT, "profiles", "r07_stat_pairs_e2e.txt")
rows_e2e.__file__ = os.path.abspath(__file__)      # measure() starts THIS script's children for the calls alone


def time_pair_calls(eng, label, n, d_names, n_name_bytes, heads, counts, in_bytes, reps=5):
    """the calls of wga_stat_pairs and wga_stat_pair_rows alone (stands in for gpu_stat_rows_e2e.time_two_calls in the children)"""
    from wgatools_amd import engine
    d_heads = eng.upload(heads)
    work = eng.empty(int(eng.lib.wga_stat_pairs_work_bytes(n)), np.uint8)
    n_pairs = C.c_uint64(0)
    args = (eng.ctx, n, d_names.ptr, n_name_bytes, d_heads.ptr, counts.ptr, work.ptr, C.byref(n_pairs))

    def timed(call, reps=reps):
        t = []
        for _ in range(reps + 1):                  # the first one warms up
            eng.sync()
            t0 = time.perf_counter()
            eng._check(call())
            eng.sync()
            t.append(time.perf_counter() - t0)
        return min(t[1:])

    t_group = timed(lambda: eng.lib.wga_stat_pairs(*args, None, None, None, 0))
    np_ = int(n_pairs.value)
    d_pairs, d_por = eng.empty(np_, engine.STAT_PAIR_DTYPE), eng.empty(n, np.uint32)
    other = eng.empty(np_, engine.STAT_PAIR_DTYPE)
    flip = [0]

    def sums():                                    # another output array every time: the whole second call, never the repeat
        flip[0] ^= 1
        return eng.lib.wga_stat_pairs(*args, d_por.ptr, None, (d_pairs, other)[flip[0]].ptr, np_)
    t_sums = timed(sums)
    eng._check(eng.lib.wga_stat_pairs(*args, d_por.ptr, None, d_pairs.ptr, np_))
    d_inv = eng.upload(np.full(np_, 0x3F800000, dtype=np.uint32))
    t_fold = timed(lambda: eng.lib.wga_stat_pairs(*args, d_por.ptr, d_inv.ptr, d_pairs.ptr, np_))
    print("the calls of wga_stat_pairs (%s): %d records, %d pairs, %.1f MB of workspace" % (
        label, n, np_, int(eng.lib.wga_stat_pairs_work_bytes(n)) / 1e6))
    print("    first call  %.3f ms best of %d (host clock: table rounds with a read-back each, scans, sort)" % (t_group * 1e3, reps))
    print("    second call %.3f ms best of %d (init, reduce over %.1f MB of counters, fold)" % (t_sums * 1e3, reps, 88 * n / 1e6))
    print("    repeat with d_inv_in %.3f ms best of %d (the fold alone)" % (t_fold * 1e3, reps))
    pairs = d_pairs.numpy()
    h = heads[pairs["first_rec"].astype(np.int64)].copy()
    h["ref_start"], h["query_start"] = pairs["ref_start"], pairs["query_start"]
    d_ph, d_sums = eng.upload(h), eng.upload(np.ascontiguousarray(pairs["sum"]))
    d_bits = eng.upload(np.ascontiguousarray(pairs["inv_size_bits"]))
    rwork = eng.empty(int(eng.lib.wga_stat_rows_work_bytes(np_)), np.uint8)
    row_off = eng.empty(np_ + 1, np.uint64)
    total = C.c_uint64(0)
    rargs = (eng.ctx, np_, d_names.ptr, n_name_bytes, d_ph.ptr, d_sums.ptr, d_bits.ptr, rwork.ptr, row_off.ptr, C.byref(total))
    t_count = timed(lambda: eng.lib.wga_stat_pair_rows(*rargs, None))
    out = eng.empty(int(total.value) + 16, np.uint8)
    t_fill = timed(lambda: eng.lib.wga_stat_pair_rows(*rargs, out.ptr))
    print("    wga_stat_pair_rows: count %.3f ms, fill %.3f ms for %d rows, %.2f MB of text" % (
        t_count * 1e3, t_fill * 1e3, np_, total.value / 1e6))


rows_e2e.time_two_calls = time_pair_calls


def own_pairs(src, dst):
    """every record its own pair: the record's number behind the query name"""
    with open(src, "rb") as f, open(dst, "wb") as g:
        for k, ln in enumerate(f):
            q, rest = ln.split(b"\t", 1)
            g.write(q + b"_%d\t" % k + rest)


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--probe":
        return probe()
    if len(sys.argv) > 1 and sys.argv[1] == "--two-calls-paf":
        return rows_e2e.two_calls_paf(sys.argv[2])
    if len(sys.argv) > 1 and sys.argv[1] == "--two-calls-maf":
        return rows_e2e.two_calls_maf(sys.argv[2])
    scale = int(sys.argv[1]) if len(sys.argv) > 1 else 1
    from wgatools_amd import build
    me = os.path.abspath(__file__)
    ok = False
    report = rows_e2e.Report()
    if not os.path.exists(build.CLI_BIN) or child([sys.executable, me, "--probe"], 120)[0] != 0:
        report.append("no MI355X visible (or wgatools not built): this file holds no figures")
    else:
        work = sys.argv[2] if len(sys.argv) > 2 else tempfile.mkdtemp(prefix="stat_pairs_e2e_")
        parent = os.environ.get("WGA_PARENT_CLI")
        if not (parent and os.path.exists(parent)):
            report.append("WGA_PARENT_CLI not set: the parent commit's binary is NOT measured")
            parent = None
        n_rec, mean_ops = max(1, rows_e2e.PAF_SHAPE[0] // scale), rows_e2e.PAF_SHAPE[1]
        paf, own = os.path.join(work, "in.paf"), os.path.join(work, "in_own.paf")
        t0 = time.perf_counter()
        rc, _, err, _ = child([sys.executable, os.path.join(ROOT, "scripts", "gpu_paf2maf_frame_e2e.py"), "--make", str(n_rec),
                               str(mean_ops), work], rows_e2e.LIMIT_S)
        if rc != 0:
            report.append("making the PAF failed (exit %d): %s" % (rc, err.strip()[-300:]))
        else:
            report.append("stat -f paf file to file: %d records of %d ops in the mean, %.2f GB of PAF (made in %.0f s); %.0f GB free in "
                          "the work directory" % (n_rec, mean_ops, os.path.getsize(paf) / 1e9, time.perf_counter() - t0,
                                                  shutil.disk_usage(work).free / 1e9))
            ok = rows_e2e.measure(report, "stat -f paf, %d x %d, the generator's names" % (n_rec, mean_ops), ["stat", "-f", "paf"], paf,
                                  work, parent, "--two-calls-paf")
            if ok:
                own_pairs(paf, own)
                report.append("stat -f paf file to file, every record its own pair")
                ok = rows_e2e.measure(report, "stat -f paf, %d x %d, every record its own pair" % (n_rec, mean_ops),
                                      ["stat", "-f", "paf"], own, work, parent, "--two-calls-paf")
        for f in ("in.paf", "in_own.paf", "t.fa", "q.fa"):
            if os.path.exists(os.path.join(work, f)):
                os.remove(os.path.join(work, f))
        if ok:
            maf = os.path.join(work, "in.maf")
            t0 = time.perf_counter()
            n_blocks = maf_e2e.write_maf(maf, max(1, rows_e2e.MAF_COPIES // scale))
            report.append("stat file to file: %d blocks of %d columns, %.2f GB of MAF (written in %.0f s)" % (
                n_blocks, maf_e2e.COLS, os.path.getsize(maf) / 1e9, time.perf_counter() - t0))
            ok = rows_e2e.measure(report, "stat on MAF, %d blocks" % n_blocks, ["stat"], maf, work, parent, "--two-calls-maf")
            if os.path.exists(maf):
                os.remove(maf)
    with open(OUT, "w") as f:
        f.write("\n".join(report) + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
