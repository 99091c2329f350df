"""`maf2chain` and `paf2chain` file to file, at the sizes of configs[2] and configs[1]: the MAF of scripts/gpu_maf2paf_e2e.py
(2 000 000 blocks x 1 500 columns x 2 rows) and the PAF of scripts/gpu_paf_filter_e2e.py (100 000 records x mean 5 000 ops), both
made with numpy here (this process never opens the GPU).  Each command is run three ways: this tree (K30 writes the chain heads:
the device writer) three times, the parent commit's `wgatools` binary five times when WGA_PARENT_CLI names it (the spread of its
wall times is the margin: "faster" needs the device writer's slowest run below the parent's fastest by more than that spread, and
"slower" the same rule turned round), and this tree with WGA_CHAIN_HEAD_WRITER=host (the heads from one host thread, as before
K30).  All under WGA_TIMING=1, one process on the GPU at a time (the probe and the kernel timing are children too), each under its
own time limit; the first step that fails ends the script.  The outputs of a command must be equal byte for byte.  Then both
calls of wga_chain_heads alone, in a child process, on the records of the PAF's first piece: the count call and the fill call
timed around a synchronise, with the bytes of heads and record ends the fill wrote.
Wall times, phase lines and the two calls' bytes and times go to profiles/r07_chain_heads_e2e.txt.  Without a visible MI355X the
file says so and holds no figure.
Usage: python scripts/gpu_chain_heads_e2e.py [COPIES] [RECORDS] [WORKDIR]   (default 20 copies of 100 000 blocks, 100 000 records,
a temporary directory)"""
import ctypes as C
import filecmp
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
from gpu_maf2paf_e2e import COLS, child, probe, write_maf  # noqa: E402
from gpu_paf_filter_e2e import write_paf_file              # noqa: E402

OUT = os.path.join(ROOT, "profiles", "r07_chain_heads_e2e.txt")
LIMIT_S, PARENT_RUNS = 300, 5
PIECE = 192 << 20


def two_calls(src, reps=5):
    """a child: the records of the PAF's first piece through the splitter, the tokeniser and K10's count call, then both calls of
    wga_chain_heads, each timed"""
    import torch  # noqa: F401
    from wgatools_amd import build, engine, _lib
    eng = engine.Engine(0, _lib.load(build.HIP_LIB))
    with open(src, "rb") as f:
        data = f.read(PIECE)
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
    trim, nbytes, diag = eng.cigar_chain(batch)
    heads = np.zeros(n, dtype=engine.MAF2PAF_HEAD_DTYPE)
    heads["q"], heads["t"], heads["strand_neg"] = ln["num"][:, 0:3], ln["num"][:, 3:6], ln["strand_neg"]
    for side in ("q", "t"):
        heads[side + "name_off"], heads[side + "name_len"] = ln[side + "name_off"], ln[side + "name_len"]
    d_heads = eng.upload(heads)
    work = eng.empty(int(eng.lib.wga_chain_heads_work_bytes(n)), np.uint8)
    data_off = eng.empty(n, np.uint64)
    args = (n, d_text, len(data), d_heads, trim, nbytes, diag, 0)
    t_count = []
    for _ in range(reps + 1):                      # the first one warms up
        eng.sync()
        t0 = time.perf_counter()
        total, good = eng.chain_heads_count(*args, work, data_off)
        t_count.append(time.perf_counter() - t0)
    out = eng.empty(total + 16, np.uint8)
    c_total, c_good = C.c_uint64(total), C.c_uint32(good)
    t_fill = []
    for _ in range(reps + 1):
        eng.sync()
        t0 = time.perf_counter()
        eng._check(eng.lib.wga_chain_heads(eng.ctx, n, d_text.ptr, len(data), d_heads.ptr, trim.ptr, nbytes.ptr, diag.ptr, 0, work.ptr,
                                           data_off.ptr, C.byref(c_total), C.byref(c_good), out.ptr))
        eng.sync()
        t_fill.append(time.perf_counter() - t0)
    written = total - int(nbytes.numpy()[:good].sum())
    best = min(t_fill[1:])
    print("both calls of wga_chain_heads: %d records (%d good), %d ops, %.1f MB of PAF, %.1f MB of chain text of which %.3f MB are "
          "heads and record ends (%.2f %%), %.2f MB of workspace" % (n, good, n_ops, len(data) / 1e6, total / 1e6, written / 1e6,
                                                                     100.0 * written / max(total, 1),
                                                                     int(eng.lib.wga_chain_heads_work_bytes(n)) / 1e6))
    print("    count call %.3f ms best of %d (host clock; plan, scan of %d records, places, one 16-byte copy back)" % (
        min(t_count[1:]) * 1e3, reps, n))
    print("    fill call  %.3f ms best of %d (host clock around a synchronise): %.2f GB/s of heads and record ends written" % (
        best * 1e3, reps, written / best / 1e9))
    eng.close()
    return 0


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--probe":
        return probe()
    if len(sys.argv) > 1 and sys.argv[1] == "--two-calls":
        return two_calls(sys.argv[2])
    copies = int(sys.argv[1]) if len(sys.argv) > 1 else 20
    n_rec = int(sys.argv[2]) if len(sys.argv) > 2 else 100_000
    from wgatools_amd import build
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
        work = sys.argv[3] if len(sys.argv) > 3 else tempfile.mkdtemp(prefix="chain_heads_e2e_")
        parent = os.environ.get("WGA_PARENT_CLI")
        if not (parent and os.path.exists(parent)):
            report.append("WGA_PARENT_CLI not set: the parent commit's binary is NOT measured")
            parent = None
        ok = True
        paf = os.path.join(work, "in.paf")
        for cmd in ("maf2chain", "paf2chain"):
            src = os.path.join(work, "in.maf" if cmd == "maf2chain" else "in.paf")
            t0 = time.perf_counter()
            if cmd == "maf2chain":
                n_blocks = write_maf(src, copies)
                report.append("maf2chain file to file: %d blocks of %d columns, %.2f GB of MAF (written in %.0f s)" % (
                    n_blocks, COLS, os.path.getsize(src) / 1e9, time.perf_counter() - t0))
            else:
                write_paf_file(src, n_rec)
                report.append("paf2chain file to file: %d records of 5 000 ops in the mean, %.2f GB of PAF (written in %.0f s)" % (
                    n_rec, os.path.getsize(src) / 1e9, time.perf_counter() - t0))
            ways = [("this tree (device writer)", build.CLI_BIN, {}, 3)]
            if parent:
                ways.append(("parent commit's binary", parent, {}, PARENT_RUNS))
            ways.append(("this tree, WGA_CHAIN_HEAD_WRITER=host", build.CLI_BIN, {"WGA_CHAIN_HEAD_WRITER": "host"}, 1))
            outs, spans = [], {}
            for name, cli, env, runs in ways:
                dst = os.path.join(work, "out_%d.chain" % len(outs))
                walls = []
                for k in range(runs):
                    rc, _, err, wall = child([cli, cmd, src, "-o", dst, "-r"], LIMIT_S, dict(env, WGA_TIMING="1"))
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
                    spans[cli] = (min(walls), max(walls))
                outs.append(dst)
            if ok and parent in spans:
                dev, par = spans[build.CLI_BIN], spans[parent]
                margin = par[1] - par[0]
                report.append("  %s: device writer %.3f .. %.3f s, parent %.3f .. %.3f s, parent's spread %.3f s: faster beyond the "
                              "spread: %s, slower beyond the spread: %s" % (cmd, dev[0], dev[1], par[0], par[1], margin,
                                                                            dev[1] < par[0] - margin, dev[0] > par[1] + margin))
            if ok:
                same = all(filecmp.cmp(outs[0], o, shallow=False) for o in outs[1:])
                report.append("  outputs equal (%d files): %s" % (len(outs), same))
                ok = same
            for p in outs:
                if os.path.exists(p):
                    os.remove(p)
            if cmd == "maf2chain" and os.path.exists(src):
                os.remove(src)
            if not ok:
                break
        if ok:
            rc, text, err, _ = child([sys.executable, me, "--two-calls", paf], LIMIT_S)
            report.extend(text.strip().split("\n"))
            if rc != 0:
                report.append("the two calls' step failed (exit %d): %s" % (rc, err.strip()[-300:]))
                ok = False
        if os.path.exists(paf):
            os.remove(paf)
    text = "\n".join(report) + "\n"
    with open(OUT, "w") as f:
        f.write(text)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
