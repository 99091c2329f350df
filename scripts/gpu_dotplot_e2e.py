"""`dotplot -f paf --out-format csv -l 0` file to file: the synthetic PAF of scripts/gpu_paf_filter_e2e.py (N records with cg:Z:
tags of a mean of 5 000 ops; configs[1]'s 100 000 records and 5·10⁸ ops at the default N), every insertion and deletion a row, three ways:
this tree (K12 makes the segments, K26 writes their rows: the device writer), this tree with WGA_DOTPLOT_WRITER=host (the
segments downloaded and printed by one CPU thread, unchanged) and, when WGA_PARENT_CLI names it, the parent commit's `wgatools`
binary, that one five times: the spread of its wall times is the margin the device writer has to beat.  All under WGA_TIMING=1,
one process on the GPU at a time (this process itself never opens it: the probe and the kernel timing are children too), each
under its own time limit; the first step that fails ends the script.  The three outputs must be equal byte for byte.  Then the
fill call alone, in a child process: the first piece of the file (at most 192 MB, cut at a line end) through K13, the span
tokeniser and K12, then both calls of wga_dotplot_csv, the fill call timed around a synchronise.  Wall times, phase lines, the
row count, the output bytes and the fill call's time and bytes per second go to profiles/r07_dotplot_e2e.txt.  Without a visible
MI355X the file says so and holds no figure.
What to compare: the whole command with the parent's wall times on the same file and box; the fill call (bytes written per
second) with the 5.85 TB/s of a plain copy and the 0.145 TB/s of K25's fill (profiles/r07_chain_filter_e2e.txt).
Usage: python scripts/gpu_dotplot_e2e.py [N_RECORDS] [WORKDIR]      (default 100 000 records, a temporary directory)"""
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
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "profiles", "r07_dotplot_e2e.txt")
LIMIT_S, DEVICE_RUNS, PARENT_RUNS = 600, 3, 5
PIECE = 192 << 20


def child(args, limit, env=None):
    """one process under its own time limit: (exit status, stdout, stderr, wall seconds)"""
    t0 = time.perf_counter()
    r = subprocess.run(["timeout", "-k", "10", str(limit)] + args, env=dict(os.environ, **(env or {})), stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE)
    return r.returncode, r.stdout.decode(errors="replace"), r.stderr.decode(errors="replace"), time.perf_counter() - t0


def probe():
    """a child: is there a device?"""
    from wgatools_amd import build
    if not os.path.exists(build.HIP_LIB):
        return 1
    import torch  # noqa: F401  first: the library then shares torch's HIP runtime
    try:
        return 0 if C.CDLL(build.HIP_LIB).wga_device_count() > 0 else 1
    except OSError:
        return 1


def fill_kernel(src, reps=5):
    """a child: the segments of the first piece as the command makes them, then both calls of wga_dotplot_csv, the fill call timed"""
    import torch  # noqa: F401
    from wgatools_amd import build, engine, _lib
    eng = engine.Engine(0, _lib.load(build.HIP_LIB))
    with open(src, "rb") as f:
        data = f.read(PIECE)
    data = data[:data.rindex(b"\n") + 1]
    d_text = eng.upload(np.frombuffer(data + b"\0" * 16, dtype=np.uint8))
    n = eng.paf_split(d_text, len(data))
    d_lines = eng.empty(n + 1, engine.PAF_LINE_DTYPE)
    eng.paf_split(d_text, len(data), d_lines)
    lines = d_lines.numpy()[:n]
    beg, end = eng.upload(lines["cg_beg"].astype(np.uint64)), eng.upload(lines["cg_end"].astype(np.uint64))
    op_cnt, err = eng.cigar_tokenise_spans(n, d_text, beg, end)
    op_off = eng.exclusive_scan_u64(n, op_cnt)
    n_ops = int(op_off.numpy()[-1])
    ops = eng.empty(n_ops + 4, np.uint32)
    eng.cigar_tokenise_spans(n, d_text, beg, end, op_cnt=op_cnt, err=err, ops=ops, op_off=op_off)
    batch = eng.make_batch_device(ops, op_off, eng.upload(lines["strand_neg"].astype(np.uint8)), n, n_ops)
    d_ts, d_qs = eng.upload(lines["num"][:, 4].astype(np.uint64)), eng.upload(lines["num"][:, 1].astype(np.uint64))
    cnt = eng.cigar_dotplot(batch, 0, d_ts, d_qs)
    seg_off = eng.exclusive_scan_u64(n, cnt)
    n_rows = int(seg_off.numpy()[-1])
    segs = eng.empty((n_rows + 1) * 5, np.uint64)
    eng.cigar_dotplot(batch, 0, d_ts, d_qs, segs=segs, seg_off=seg_off)
    tails = [b"," + data[int(l["tname_off"]):int(l["tname_off"]) + int(l["tname_len"])] + b"," +
             data[int(l["qname_off"]):int(l["qname_off"]) + int(l["qname_len"])] + b"\n" for l in lines]      # names without a comma or a quote
    d_tails = eng.upload(np.frombuffer(b"".join(tails), dtype=np.uint8))
    d_tail_off = eng.upload(np.cumsum([0] + [len(t) for t in tails]).astype(np.uint64))
    work = eng.empty(int(eng.lib.wga_dotplot_csv_work_bytes(n_rows)), np.uint8)
    eng.sync()
    t0 = time.perf_counter()
    total = eng.dotplot_csv_count(n, segs, seg_off, d_tails, d_tail_off, work)
    t_count = time.perf_counter() - t0
    out = eng.empty(total + 16, np.uint8)
    c_total = C.c_uint64(total)
    times = []
    for _ in range(reps + 1):                      # the first one warms up
        eng.sync()
        t0 = time.perf_counter()
        eng._check(eng.lib.wga_dotplot_csv(eng.ctx, n, segs.ptr, seg_off.ptr, d_tails.ptr, d_tail_off.ptr, work.ptr, C.byref(c_total), out.ptr))
        eng.sync()
        times.append(time.perf_counter() - t0)
    best = min(times[1:])
    print("fill call on the first piece: %d records, %.1f MB of PAF text, %d ops, %d rows (%.1f MB of segments), %.1f MB of csv out" % (
        n, len(data) / 1e6, n_ops, n_rows, n_rows * 40 / 1e6, total / 1e6))
    print("    count call %.3f ms (host clock; sizes, scan of %d rows, two small copies back)" % (t_count * 1e3, n_rows))
    print("    fill call  %.3f ms best of %d (host clock around a synchronise, one 8-byte copy in front): %.3f TB/s of text written"
          % (best * 1e3, reps, total / best / 1e12))
    eng.close()
    return 0


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--probe":
        return probe()
    if len(sys.argv) > 1 and sys.argv[1] == "--fill-kernel":
        return fill_kernel(sys.argv[2])
    n_records = int(sys.argv[1]) if len(sys.argv) > 1 else 100000
    from wgatools_amd import build
    from gpu_paf_filter_e2e import write_paf_file
    me = os.path.abspath(__file__)
    ok = False

    class Report(list):          # every line is shown as it comes: a long run is not silent
        def append(self, ln):
            list.append(self, ln)
            print(ln, flush=True)

        def extend(self, lns):
            for ln in lns:
                self.append(ln)
    report = Report()
    if not os.path.exists(build.CLI_BIN) or child([sys.executable, me, "--probe"], 120)[0] != 0:
        report.append("no MI355X visible (or wgatools not built): no figures")
    else:
        work = sys.argv[2] if len(sys.argv) > 2 else tempfile.mkdtemp(prefix="dotplot_e2e_")
        src = os.path.join(work, "in.paf")
        write_paf_file(src, n_records)
        report.append("dotplot -f paf --out-format csv -l 0 file to file: %d records, %.1f MB of PAF text" % (
            n_records, os.path.getsize(src) / 1e6))
        if n_records != 100000:
            report.append("  (configs[1]'s size is 100 000 records: this run is at %.2f of it)" % (n_records / 100000))
        parent = os.environ.get("WGA_PARENT_CLI")
        ways = [("this tree (device writer)", build.CLI_BIN, {}, DEVICE_RUNS),
                ("this tree, WGA_DOTPLOT_WRITER=host", build.CLI_BIN, {"WGA_DOTPLOT_WRITER": "host"}, 1)]
        if parent and os.path.exists(parent):
            ways.append(("parent commit's binary", parent, {}, PARENT_RUNS))
        else:
            report.append("WGA_PARENT_CLI not set: the parent commit's binary is NOT measured")
        ok = True
        outs = []
        for name, cli, env, runs in ways:
            dst = os.path.join(work, "out_%d.csv" % len(outs))
            walls = []
            for k in range(runs):
                rc, _, err, wall = child([cli, "dotplot", "-f", "paf", "--out-format", "csv", "-l", "0", src, "-o", dst, "-r"], LIMIT_S,
                                         dict(env, WGA_TIMING="1"))
                walls.append(wall)
                report.append("  %s%s: exit %d, wall %.3f s, %.1f MB out" % (
                    name, " (run %d)" % (k + 1) if runs > 1 else "", rc, wall, os.path.getsize(dst) / 1e6 if os.path.exists(dst) else 0.0))
                report.extend("      " + ln for ln in err.strip().split("\n"))
                if rc != 0:                            # nothing more is started on the device behind a failed step
                    report.append("step failed: the run ends here")
                    ok = False
                    break
            if not ok:
                break
            if runs > 1:
                report.append("  %s: wall min %.3f s, median %.3f s, max %.3f s over %d runs" % (
                    name, min(walls), float(np.median(walls)), max(walls), runs))
            outs.append(dst)
        if ok:
            with open(outs[0], "rb") as f:
                rows = sum(chunk.count(b"\n") for chunk in iter(lambda: f.read(1 << 24), b"")) - 1      # without the header line
            report.append("  %d rows, %d bytes of csv" % (rows, os.path.getsize(outs[0])))
            same = all(filecmp.cmp(outs[0], o, shallow=False) for o in outs[1:])
            report.append("  outputs equal: %s" % same)
            ok = same
        for p in outs:
            if os.path.exists(p):
                os.remove(p)
        if ok:
            rc, text, err, _ = child([sys.executable, me, "--fill-kernel", src], LIMIT_S)
            report.extend(text.strip().split("\n"))
            if rc != 0:
                report.append("fill call step failed (exit %d): %s" % (rc, err.strip()[-300:]))
                ok = False
        if os.path.exists(src):
            os.remove(src)
    text = "\n".join(report) + "\n"
    with open(OUT, "w") as f:
        f.write(text)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
