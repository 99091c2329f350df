"""`maf-index` file to file on configs[2]'s MAF (2 000 000 blocks of 1 500 columns, written with numpy as
scripts/gpu_maf2paf_e2e.py does; this process never opens the GPU), three ways: this tree (K35 builds the entries: the device
writer) three times, the parent commit's `wgatools` binary five times when WGA_PARENT_CLI names it, and this tree with
WGA_MAF_INDEX_WRITER=host once.  The parent's spread of wall times is the margin: "faster" needs the device writer's slowest run
below the parent's fastest by more than that spread, "slower" is the same rule turned round, and if neither holds the answer is "not
shown".  All under WGA_TIMING=1, one process on the GPU at a time (the probe and the kernel timing are children too), each under
its own time limit; the first step that fails ends the script.  The indices must be equal byte for byte.  Then both calls of
wga_maf_index alone, in a child process, on the lines of the file's first GiB: the count call and the fill call timed around a
synchronise, the fill's rate next to K33's 0.36 TB/s (profiles/r07_stat_rows_e2e.txt).
Wall times, phase lines and the two calls' bytes and times go to profiles/r07_maf_index_e2e.txt.  Without a visible MI355X the file
says that it holds no figures.
Usage: python scripts/gpu_maf_index_e2e.py [SCALE] [WORKDIR]   (SCALE divides the block count, default 1; default a temporary
directory)"""
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

OUT = os.path.join(ROOT, "profiles", "r07_maf_index_e2e.txt")
LIMIT_S, PARENT_RUNS = 300, 5
MAF_COPIES = 20                      # x 100 000 blocks
K33_TBS = 0.36


def two_calls(src, reps=5):
    """a child: the splitter on the file's first GiB, then both calls of wga_maf_index, each timed"""
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
    work_bytes = int(eng.lib.wga_maf_index_work_bytes(nl))
    work = eng.empty(work_bytes, np.uint8)
    host = [C.c_uint64(0) for _ in range(7)]
    args = (eng.ctx, d_text.ptr, len(data), d_lines.ptr, nl, 0, 0, 0, work.ptr) + tuple(C.byref(v) for v in host)
    t_count = []
    for _ in range(reps + 1):                                      # the first one warms up
        eng.sync()
        t0 = time.perf_counter()
        eng._check(eng.lib.wga_maf_index(*args, None, None))
        t_count.append(time.perf_counter() - t0)
    n_names, n_blocks, n_slines, total = (int(v.value) for v in host[:4])
    out = eng.empty(total + 16, np.uint8)
    names = eng.empty((n_names + 1) * 48, np.uint8)
    t_fill = []
    for _ in range(reps + 1):
        eng.sync()
        t0 = time.perf_counter()
        eng._check(eng.lib.wga_maf_index(*args, names.ptr, out.ptr))
        eng.sync()
        t_fill.append(time.perf_counter() - t0)
    best = min(t_fill[1:])
    print("both calls of wga_maf_index (the MAF's first GiB): %d lines, %d s-lines in %d blocks, %d names, %.1f MB of input, "
          "%.1f MB of text (%.1f bytes an interval), %.1f MB of workspace" % (
              nl, n_slines, n_blocks, n_names, len(data) / 1e6, total / 1e6, total / max(n_slines, 1), work_bytes / 1e6))
    print("    count call %.3f ms best of %d (host clock; newline list, scans, the name table's rounds, the sort, the intervals' scan)" % (
        min(t_count[1:]) * 1e3, reps))
    print("    fill call  %.3f ms best of %d (host clock around a synchronise): %.3f TB/s of text written (K33's rows: %.2f TB/s)" % (
        best * 1e3, reps, total / best / 1e12, K33_TBS))
    eng.close()
    return 0


class Report(list):          # every line is shown as it comes: a long run is not silent
    def append(self, ln):
        list.append(self, ln)
        print(ln, flush=True)

    def extend(self, lns):
        for ln in lns:
            self.append(ln)


def measure(report, what, src, work, parent):
    """the three ways, the verdict, the indices' comparison, the two calls; False when a step failed"""
    from wgatools_amd import build
    me = os.path.abspath(__file__)
    ways = [("this tree (device writer)", build.CLI_BIN, {}, 3)]
    if parent:
        ways.append(("parent commit's binary", parent, {}, PARENT_RUNS))
    ways.append(("this tree, WGA_MAF_INDEX_WRITER=host", build.CLI_BIN, {"WGA_MAF_INDEX_WRITER": "host"}, 1))
    first, dst = os.path.join(work, "first.index"), os.path.join(work, "out.index")
    spans, same, compared = {}, True, 0
    for name, cli, env, runs in ways:
        walls = []
        for k in range(runs):
            to = dst if os.path.exists(first) else first       # the first index stays: the others are compared with it and go
            rc, _, err, wall = child([cli, "-o", to, "maf-index", src], LIMIT_S, dict(env, WGA_TIMING="1"))
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
            "faster beyond the spread" if faster else "slower beyond the spread" if slower else "not shown to be faster or slower"))
    report.append("  indices equal (%d files against the first): %s" % (compared, same))
    if os.path.exists(first):
        os.remove(first)
    if not same:
        return False
    rc, text, err, _ = child([sys.executable, me, "--two-calls", src], LIMIT_S)
    report.extend(text.strip().split("\n"))
    if rc != 0:
        report.append("the two calls' step failed (exit %d): %s" % (rc, err.strip()[-300:]))
        return False
    return True


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--probe":
        return probe()
    if len(sys.argv) > 1 and sys.argv[1] == "--two-calls":
        return two_calls(sys.argv[2])
    scale = int(sys.argv[1]) if len(sys.argv) > 1 else 1
    from wgatools_amd import build
    me = os.path.abspath(__file__)
    ok = False
    report = Report()
    if not os.path.exists(build.CLI_BIN) or child([sys.executable, me, "--probe"], 120)[0] != 0:
        report.append("no MI355X visible (or wgatools not built): this file holds no figures")
    else:
        work = sys.argv[2] if len(sys.argv) > 2 else tempfile.mkdtemp(prefix="maf_index_e2e_")
        parent = os.environ.get("WGA_PARENT_CLI")
        if not (parent and os.path.exists(parent)):
            report.append("WGA_PARENT_CLI not set: the parent commit's binary is NOT measured")
            parent = None
        maf = os.path.join(work, "in.maf")
        t0 = time.perf_counter()
        n_blocks = maf_e2e.write_maf(maf, max(1, MAF_COPIES // scale))
        report.append("maf-index file to file: %d blocks of %d columns, %.2f GB of MAF (written in %.0f s); %.0f GB free in the work "
                      "directory" % (n_blocks, maf_e2e.COLS, os.path.getsize(maf) / 1e9, time.perf_counter() - t0,
                                     shutil.disk_usage(work).free / 1e9))
        ok = measure(report, "maf-index, %d blocks" % n_blocks, maf, work, parent)
        if os.path.exists(maf):
            os.remove(maf)
    text = "\n".join(report) + "\n"
    with open(OUT, "w") as f:
        f.write(text)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
