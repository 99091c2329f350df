"""`dotplot -m overview --out-format csv` file to file at the two shapes the project measures elsewhere: `-f paf` on the
short-record PAF of scripts/gpu_paf2maf_frame_e2e.py (1 000 000 records x mean 500 ops, made by that script's input maker in a
child process), and on configs[2]'s MAF (2 000 000 blocks of 1 500 columns, written with numpy as scripts/gpu_maf2paf_e2e.py
does; this process never opens the GPU).  Each shape is run three ways: this tree (K34 writes the rows: the device writer) three
times, the parent commit's `wgatools` binary five times when WGA_PARENT_CLI names it, and this tree with WGA_DOTPLOT_WRITER=host
once.  The parent's spread of wall times is the margin: "faster" needs the device writer's slowest run below the parent's fastest
by more than that spread, "slower" is the same rule turned round, and if neither holds the answer is "NOT shown to be faster".
All under WGA_TIMING=1, one process on the GPU at a time (the probe, the input maker and the kernel timing are children too),
each under its own time limit; the first step that fails ends the script.  The outputs of a shape must be equal byte for byte.
Then both calls of wga_dotplot_overview alone, in a child process, on the records of the file's first piece: the count call and
the fill call timed around a synchronise, the fill's rate next to K33's 0.36 TB/s (profiles/r07_stat_rows_e2e.txt).
Wall times, phase lines and the two calls' bytes and times go to profiles/r07_dotplot_overview_e2e.txt.  Without a visible MI355X
the file says that it holds no figures.
Usage: python scripts/gpu_dotplot_overview_e2e.py [SCALE] [WORKDIR]   (SCALE divides both shapes' record counts, default 1;
default a temporary directory)"""
import ctypes as C
import filecmp
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
from gpu_maf2paf_e2e import child, probe  # noqa: E402
from gpu_stat_rows_e2e import Report  # noqa: E402

OUT = os.path.join(ROOT, "profiles", "r07_dotplot_overview_e2e.txt")
LIMIT_S, PARENT_RUNS = 300, 5
PAF_SHAPE = (1_000_000, 500)
MAF_COPIES = 20                      # x 100 000 blocks
K33_TBS = 0.36
ARGS = ["dotplot", "-m", "overview", "--out-format", "csv"]
HOST_WRITER = {"WGA_DOTPLOT_WRITER": "host"}


def time_two_calls(eng, label, n, d_names, n_name_bytes, heads, counts, in_bytes, reps=5):
    d_heads = eng.upload(heads)
    work = eng.empty(int(eng.lib.wga_dotplot_overview_work_bytes(n)), np.uint8)
    row_off = eng.empty(n + 1, np.uint64)
    c_total = C.c_uint64(0)
    args = (eng.ctx, n, d_names.ptr, n_name_bytes, d_heads.ptr, counts.ptr, 0, work.ptr, row_off.ptr, C.byref(c_total))
    t_count = []
    for _ in range(reps + 1):                      # the first one warms up
        eng.sync()
        t0 = time.perf_counter()
        eng._check(eng.lib.wga_dotplot_overview(*args, None))
        t_count.append(time.perf_counter() - t0)
    total = int(c_total.value)
    out = eng.empty(total + 16, np.uint8)
    t_fill = []
    for _ in range(reps + 1):
        eng.sync()
        t0 = time.perf_counter()
        eng._check(eng.lib.wga_dotplot_overview(*args, out.ptr))
        eng.sync()
        t_fill.append(time.perf_counter() - t0)
    best = min(t_fill[1:])
    print("both calls of wga_dotplot_overview (%s): %d rows, %.1f MB of input, %.1f MB of text (%.1f bytes a row), %.1f MB of "
          "workspace" % (label, n, in_bytes / 1e6, total / 1e6, total / max(n, 1), int(eng.lib.wga_dotplot_overview_work_bytes(n)) / 1e6))
    print("    count call %.3f ms best of %d (host clock; plan, scan of %d rows, one 8-byte copy back)" % (min(t_count[1:]) * 1e3, reps, n))
    print("    fill call  %.3f ms best of %d (host clock around a synchronise): %.3f TB/s of text written (K33's rows: %.2f TB/s)" % (
        best * 1e3, reps, total / best / 1e12, K33_TBS))


def two_calls_paf(src):
    """a child: the records of the PAF's first piece through the splitter, the tokeniser and K1, then both calls of
    wga_dotplot_overview"""
    import torch  # noqa: F401
    from wgatools_amd import build, engine, _lib
    eng = engine.Engine(0, _lib.load(build.HIP_LIB))
    with open(src, "rb") as f:
        data = f.read(192 << 20)
    data = data[:data.rfind(b"\n") + 1]                            # whole lines
    d_text = eng.upload(np.frombuffer(data + b"\0" * 16, dtype=np.uint8))
    nl = eng.paf_split(d_text, len(data))
    d_lines = eng.empty(nl + 1, engine.PAF_LINE_DTYPE)
    eng.paf_split(d_text, len(data), d_lines)
    ln = d_lines.numpy()[:nl]
    ln = ln[ln["status"] == engine.PAF_OK]
    n = len(ln)
    beg, end = eng.upload(np.ascontiguousarray(ln["cg_beg"])), eng.upload(np.ascontiguousarray(ln["cg_end"]))
    cnt, err = eng.cigar_tokenise_spans(n, d_text, beg, end)
    op_off = eng.exclusive_scan_u64(n, cnt)
    n_ops = int(op_off.numpy()[-1])
    ops = eng.empty(n_ops + 4, np.uint32)
    eng.cigar_tokenise_spans(n, d_text, beg, end, op_cnt=cnt, err=err, ops=ops, op_off=op_off)
    batch = eng.make_batch_device(ops, op_off, eng.upload(np.ascontiguousarray(ln["strand_neg"])), n, n_ops)
    counts, _, _ = eng.cigar_stat(batch)
    num = ln["num"].astype(np.uint64)                              # q size, start, end, t size, start, end, matches, block, mapq
    neg = ln["strand_neg"] != 0
    heads = np.zeros(n, dtype=engine.DOTPLOT_OV_HEAD_DTYPE)
    heads["ref_start"], heads["ref_end"], heads["align_size"] = num[:, 4], num[:, 5], num[:, 5] - num[:, 4]
    heads["q_first"], heads["q_second"] = np.where(neg, num[:, 2], num[:, 1]), np.where(neg, num[:, 1], num[:, 2])
    heads["rname_off"], heads["rname_len"] = ln["tname_off"], ln["tname_len"]
    heads["qname_off"], heads["qname_len"] = ln["qname_off"], ln["qname_len"]
    time_two_calls(eng, "the PAF's first piece", n, d_text, len(data), heads, counts, len(data))
    eng.close()
    return 0


def two_calls_maf(src):
    """a child: the splitter and K3 on the blocks of the file's first GiB, then both calls of wga_dotplot_overview"""
    import torch  # noqa: F401
    from wgatools_amd import build, engine, _lib
    eng = engine.Engine(0, _lib.load(build.HIP_LIB))
    with open(src, "rb") as f:
        data = f.read(1 << 30)
    data = data[:data.rfind(b"\n\n") + 2]                          # whole blocks
    d_text = eng.upload(np.frombuffer(data + b"\0" * 16, dtype=np.uint8))
    nl = eng.maf_split(d_text, len(data))
    d_lines = eng.empty(nl + 1, engine.MAF_LINE_DTYPE)
    eng.maf_split(d_text, len(data), d_lines)
    lines = d_lines.numpy()[:nl]
    s = lines[lines["status"] == 0]
    t, q = s[0::2], s[1::2]
    n = len(t)
    neg = q["strand_neg"] != 0
    qs, ql, qz = q["num"][:, 0], q["num"][:, 1], q["num"][:, 2]    # start, align_size, size
    q_lo = np.where(neg, qz - qs - ql, qs)
    heads = np.zeros(n, dtype=engine.DOTPLOT_OV_HEAD_DTYPE)
    heads["ref_start"], heads["ref_end"], heads["align_size"] = t["num"][:, 0], t["num"][:, 0] + t["num"][:, 1], t["num"][:, 1]
    heads["q_first"], heads["q_second"] = np.where(neg, q_lo + ql, q_lo), np.where(neg, q_lo, q_lo + ql)
    heads["rname_off"], heads["rname_len"] = t["name_off"], t["name_len"]
    heads["qname_off"], heads["qname_len"] = q["name_off"], q["name_len"]
    d_t, d_q = eng.upload(np.ascontiguousarray(t["seq_off"])), eng.upload(np.ascontiguousarray(q["seq_off"]))
    d_c = eng.upload(np.minimum(t["seq_len"], q["seq_len"]))
    d_s = eng.upload(neg.astype(np.uint8))
    counts, _ = eng.maf_pair_stat(n, d_text, d_t, d_q, d_c, d_s)
    time_two_calls(eng, "the MAF's first GiB", n, d_text, len(data), heads, counts, len(data))
    eng.close()
    return 0


def measure(report, what, args, src, work, parent, two_calls_flag):
    """one shape three ways, the verdict, the outputs' comparison, the two calls; False when a step failed"""
    from wgatools_amd import build
    me = os.path.abspath(__file__)
    ways = [("this tree (device writer)", build.CLI_BIN, {}, 3)]
    if parent:
        ways.append(("parent commit's binary", parent, {}, PARENT_RUNS))
    ways.append(("this tree, WGA_DOTPLOT_WRITER=host", build.CLI_BIN, HOST_WRITER, 1))
    first, dst = os.path.join(work, "out_first.csv"), os.path.join(work, "out.csv")
    spans, same, compared = {}, True, 0
    for name, cli, env, runs in ways:
        walls = []
        for k in range(runs):
            to = dst if os.path.exists(first) else first       # the first output stays: the others are compared with it and go
            rc, _, err, wall = child([cli] + args + [src, "-o", to, "-r"], LIMIT_S, dict(env, WGA_TIMING="1"))
            walls.append(wall)
            report.append("  %s%s: exit %d, wall %.3f s, %.1f MB out" % (
                name, " (run %d)" % (k + 1) if runs > 1 else "", rc, wall, os.path.getsize(to) / 1e6 if os.path.exists(to) else 0.0))
            report.extend("      " + ln for ln in err.strip().split("\n"))
            if rc != 0:                            # nothing more is started on the device behind a failed step
                report.append("step failed: the run ends here")
                return False
            if to == dst:
                same = filecmp.cmp(first, dst, shallow=False) and same
                compared += 1
                os.remove(dst)
        if runs > 1:
            report.append("  %s: wall min %.3f s, median %.3f s, max %.3f s over %d runs" % (
                name, min(walls), float(np.median(walls)), max(walls), runs))
            spans[cli] = (min(walls), max(walls))
    if parent in spans:
        dev, par = spans[build.CLI_BIN], spans[parent]
        margin = par[1] - par[0]
        faster, slower = dev[1] < par[0] - margin, dev[0] > par[1] + margin
        report.append("  %s: device writer %.3f .. %.3f s, parent %.3f .. %.3f s, parent's spread %.3f s: %s" % (
            what, dev[0], dev[1], par[0], par[1], margin,
            "faster beyond the spread" if faster else "slower beyond the spread" if slower else "NOT shown to be faster"))
    report.append("  outputs equal (%d files against the first): %s" % (compared, same))
    if os.path.exists(first):
        os.remove(first)
    if not same:
        return False
    rc, text, err, _ = child([sys.executable, me, two_calls_flag, src], LIMIT_S)
    report.extend(text.strip().split("\n"))
    if rc != 0:
        report.append("the two calls' step failed (exit %d): %s" % (rc, err.strip()[-300:]))
        return False
    return True


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--probe":
        return probe()
    if len(sys.argv) > 1 and sys.argv[1] == "--two-calls-paf":
        return two_calls_paf(sys.argv[2])
    if len(sys.argv) > 1 and sys.argv[1] == "--two-calls-maf":
        return two_calls_maf(sys.argv[2])
    scale = int(sys.argv[1]) if len(sys.argv) > 1 else 1
    from wgatools_amd import build
    me = os.path.abspath(__file__)
    ok = False
    report = Report()
    if not os.path.exists(build.CLI_BIN) or child([sys.executable, me, "--probe"], 120)[0] != 0:
        report.append("no MI355X visible (or wgatools not built): this file holds no figures")
    else:
        work = sys.argv[2] if len(sys.argv) > 2 else tempfile.mkdtemp(prefix="dotplot_overview_e2e_")
        parent = os.environ.get("WGA_PARENT_CLI")
        if not (parent and os.path.exists(parent)):
            report.append("WGA_PARENT_CLI not set: the parent commit's binary is NOT measured")
            parent = None
        # the PAF: the input maker of the paf2maf script (a child: it generates the records in HBM)
        n_rec, mean_ops = max(1, PAF_SHAPE[0] // scale), PAF_SHAPE[1]
        paf = os.path.join(work, "in.paf")
        t0 = time.perf_counter()
        rc, _, err, _ = child([sys.executable, os.path.join(ROOT, "scripts", "gpu_paf2maf_frame_e2e.py"), "--make", str(n_rec),
                               str(mean_ops), work], LIMIT_S)
        if rc != 0:
            report.append("making the PAF failed (exit %d): %s" % (rc, err.strip()[-300:]))
        else:
            report.append("dotplot -f paf -m overview file to file: %d records of %d ops in the mean, %.2f GB of PAF (made in %.0f s); "
                          "%.0f GB free in the work directory" % (n_rec, mean_ops, os.path.getsize(paf) / 1e9, time.perf_counter() - t0,
                                                                  shutil.disk_usage(work).free / 1e9))
            ok = measure(report, "dotplot -f paf -m overview, %d x %d" % (n_rec, mean_ops), ARGS + ["-f", "paf"], paf, work, parent,
                         "--two-calls-paf")
        for f in ("in.paf", "t.fa", "q.fa"):
            if os.path.exists(os.path.join(work, f)):
                os.remove(os.path.join(work, f))
        if ok:
            maf = os.path.join(work, "in.maf")
            t0 = time.perf_counter()
            n_blocks = maf_e2e.write_maf(maf, max(1, MAF_COPIES // scale))
            report.append("dotplot -m overview file to file: %d blocks of %d columns, %.2f GB of MAF (written in %.0f s)" % (
                n_blocks, maf_e2e.COLS, os.path.getsize(maf) / 1e9, time.perf_counter() - t0))
            ok = measure(report, "dotplot -m overview on MAF, %d blocks" % n_blocks, ARGS, maf, work, parent, "--two-calls-maf")
            if os.path.exists(maf):
                os.remove(maf)
    text = "\n".join(report) + "\n"
    with open(OUT, "w") as f:
        f.write(text)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
