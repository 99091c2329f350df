"""`paf2maf` file to file at two shapes of the same op count: configs[1]'s (100 000 records x mean 5 000 ops) and a short-record
shape (1 000 000 records x mean 500 ops), where the cost of the frames — which grows with the records, not with the bytes — is ten
times as large.  The inputs (a PAF and two FASTA files over 2 x 50 Mb pools) are made by a child process (the synthetic mixture of
wgatools_amd/synth.py, generated in HBM); this process never opens the GPU.  Each shape is run three ways: this tree (K32 writes
the record frames: the device writer) three times, this tree with WGA_MAF_FRAME_WRITER=host (the frames from one host thread,
scattered around the rows, as before K32), and the parent commit's `wgatools` binary five times when WGA_PARENT_CLI names it (the
spread of its wall times is the margin: "faster" needs the device writer's slowest run below the parent's fastest by more than that
spread, "slower" is the same rule turned round, and if neither holds the answer is "not shown").  All under WGA_TIMING=1, one
process on the GPU at a time (the probe, the input maker and the kernel timing are children too), each under its own time limit;
the first step that fails ends the script.  The outputs of a shape must be equal byte for byte.  Then both calls of
wga_paf2maf_frame alone, in a child process, on the records of the PAF's first piece: the count call and the fill call timed around
a synchronise, with the frame bytes the fill wrote.
Wall times, phase lines and the two calls' bytes and times go to profiles/r07_paf2maf_frame_e2e.txt.  Without a visible MI355X
the file says that it holds no figures.
Usage: python scripts/gpu_paf2maf_frame_e2e.py [SCALE] [WORKDIR]   (SCALE divides both shapes' record counts, default 1; default
a temporary directory)"""
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
from gpu_maf2paf_e2e import child, probe  # noqa: E402

OUT = os.path.join(ROOT, "profiles", "r07_paf2maf_frame_e2e.txt")
LIMIT_S, PARENT_RUNS = 300, 5
PIECE = 192 << 20
POOL = 50_000_000
SHAPES = ((100_000, 5000), (1_000_000, 500))


def make_inputs(n, mean_ops, work):
    """a child: the PAF and the two FASTA files of n records of the synthetic mixture"""
    import torch
    from wgatools_amd import synth
    tb = synth.make_paf_batch_torch(9, n, mean_ops, POOL, torch.device("cuda", 0))
    for name, key in ((b"tchr", "t_pool"), (b"qchr", "q_pool")):
        seq = tb[key].cpu().numpy().tobytes()
        with open(os.path.join(work, name.decode()[0] + ".fa"), "wb") as f:
            f.write(b">" + name + b"\n")
            for i in range(0, len(seq), 1 << 20):
                f.write(seq[i:i + (1 << 20)] + b"\n")
    synth.paf_text_torch(tb).cpu().numpy().tofile(os.path.join(work, "in.paf"))
    return 0


def two_calls(src, reps=5):
    """a child: the records of the PAF's first piece through the splitter, the tokeniser and K1, then both calls of
    wga_paf2maf_frame, each timed"""
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
    counts, diag, _ = eng.cigar_stat(batch)
    num = ln["num"].astype(np.uint64)                              # q size, start, end, t size, start, end, matches, block, mapq
    neg = ln["strand_neg"] != 0
    heads = np.zeros(n, dtype=engine.MAF_FRAME_HEAD_DTYPE)
    heads["score"] = num[:, 8]
    heads["t"] = np.stack([num[:, 4], num[:, 5] - num[:, 4], num[:, 3]], axis=1)
    heads["q"] = np.stack([np.where(neg, num[:, 0] - num[:, 2], num[:, 1]), num[:, 2] - num[:, 1], num[:, 0]], axis=1)
    heads["q_neg"] = ln["strand_neg"]
    for side in ("q", "t"):
        heads[side + "name_off"], heads[side + "name_len"] = ln[side + "name_off"], ln[side + "name_len"]
    d_heads = eng.upload(heads)
    tl, ql = eng.upload(np.ascontiguousarray(heads["t"][:, 1])), eng.upload(np.ascontiguousarray(heads["q"][:, 1]))
    work = eng.empty(int(eng.lib.wga_paf2maf_frame_work_bytes(n)), np.uint8)
    lay = eng.empty(n, np.uint64), eng.empty(n, np.uint64), eng.empty(n + 1, np.uint64)
    args = (n, d_text, len(data), d_heads, counts, tl, ql)
    t_count = []
    for _ in range(reps + 1):                      # the first one warms up
        eng.sync()
        t0 = time.perf_counter()
        total = eng.maf_frame_count(*args, work, *lay, diag=diag)
        t_count.append(time.perf_counter() - t0)
    out = eng.empty(total + 16, np.uint8)
    c_total, c_good, c_gb = C.c_uint64(total), C.c_uint32(0), C.c_uint64(0)
    t_fill = []
    for _ in range(reps + 1):
        eng.sync()
        t0 = time.perf_counter()
        eng._check(eng.lib.wga_paf2maf_frame(eng.ctx, n, d_text.ptr, len(data), d_heads.ptr, counts.ptr, tl.ptr, ql.ptr, diag.ptr,
                                             work.ptr, lay[0].ptr, lay[1].ptr, lay[2].ptr, C.byref(c_total), C.byref(c_good),
                                             C.byref(c_gb), out.ptr))
        eng.sync()
        t_fill.append(time.perf_counter() - t0)
    c = counts.numpy()
    rows = int(heads["t"][:, 1].sum() + heads["q"][:, 1].sum()) + int(sum(int(c[k].sum()) for k in ("ins_bp", "inv_ins_bp", "del_bp", "inv_del_bp")))
    written = total - rows
    best = min(t_fill[1:])
    print("both calls of wga_paf2maf_frame: %d records (%d good), %d ops, %.1f MB of PAF, %.1f MB of MAF text of which %.3f MB are "
          "frames (%.3f %%), %.2f MB of workspace" % (n, c_good.value, n_ops, len(data) / 1e6, total / 1e6, written / 1e6,
                                                     100.0 * written / max(total, 1),
                                                     int(eng.lib.wga_paf2maf_frame_work_bytes(n)) / 1e6))
    print("    count call %.3f ms best of %d (host clock; plan, scan of %d records, places, one 8-byte copy back)" % (
        min(t_count[1:]) * 1e3, reps, n))
    print("    fill call  %.3f ms best of %d (host clock around a synchronise; the fill, n_good, one 16-byte copy back): %.2f GB/s "
          "of frames written" % (best * 1e3, reps, written / best / 1e9))
    eng.close()
    return 0


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--probe":
        return probe()
    if len(sys.argv) > 1 and sys.argv[1] == "--make":
        return make_inputs(int(sys.argv[2]), int(sys.argv[3]), sys.argv[4])
    if len(sys.argv) > 1 and sys.argv[1] == "--two-calls":
        return two_calls(sys.argv[2])
    scale = int(sys.argv[1]) if len(sys.argv) > 1 else 1
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
        report.append("no MI355X visible (or wgatools not built): this file holds no figures")
    else:
        work = sys.argv[2] if len(sys.argv) > 2 else tempfile.mkdtemp(prefix="paf2maf_frame_e2e_")
        parent = os.environ.get("WGA_PARENT_CLI")
        if not (parent and os.path.exists(parent)):
            report.append("WGA_PARENT_CLI not set: the parent commit's binary is NOT measured")
            parent = None
        ok = True
        paf, t_fa, q_fa = (os.path.join(work, f) for f in ("in.paf", "t.fa", "q.fa"))
        for n_rec, mean_ops in SHAPES:
            n_rec = max(1, n_rec // scale)
            t0 = time.perf_counter()
            rc, _, err, _ = child([sys.executable, me, "--make", str(n_rec), str(mean_ops), work], LIMIT_S)
            if rc != 0:
                report.append("making the inputs failed (exit %d): %s" % (rc, err.strip()[-300:]))
                ok = False
                break
            report.append("paf2maf file to file: %d records of %d ops in the mean, %.2f GB of PAF, 2 x %d Mb of FASTA (made in %.0f s); "
                          "%.0f GB free in the work directory" % (n_rec, mean_ops, os.path.getsize(paf) / 1e9, POOL // 1_000_000,
                                                                  time.perf_counter() - t0, shutil.disk_usage(work).free / 1e9))
            ways = [("this tree (device writer)", build.CLI_BIN, {}, 3),
                    ("this tree, WGA_MAF_FRAME_WRITER=host", build.CLI_BIN, {"WGA_MAF_FRAME_WRITER": "host"}, 1)]
            if parent:
                ways.append(("parent commit's binary", parent, {}, PARENT_RUNS))
            first, dst = os.path.join(work, "out_first.maf"), os.path.join(work, "out.maf")
            spans, same, compared = {}, True, 0
            for name, cli, env, runs in ways:
                walls = []
                for k in range(runs):
                    to = dst if os.path.exists(first) else first       # the first output stays: the others are compared with it and go
                    rc, _, err, wall = child([cli, "paf2maf", paf, "-g", t_fa, "-q", q_fa, "-o", to, "-r"], LIMIT_S,
                                             dict(env, WGA_TIMING="1"))
                    walls.append(wall)
                    report.append("  %s%s: exit %d, wall %.3f s, %.1f MB out" % (
                        name, " (run %d)" % (k + 1) if runs > 1 else "", rc, wall, os.path.getsize(to) / 1e6 if os.path.exists(to) else 0.0))
                    report.extend("      " + ln for ln in err.strip().split("\n"))
                    if rc != 0:                            # nothing more is started on the device behind a failed step
                        report.append("step failed: the run ends here")
                        ok = False
                        break
                    if to == dst:
                        same = filecmp.cmp(first, dst, shallow=False) and same
                        compared += 1
                        os.remove(dst)
                if not ok:
                    break
                if runs > 1:
                    report.append("  %s: wall min %.3f s, median %.3f s, max %.3f s over %d runs" % (
                        name, min(walls), float(np.median(walls)), max(walls), runs))
                    spans[cli] = (min(walls), max(walls))
            if ok and parent in spans:
                dev, par = spans[build.CLI_BIN], spans[parent]
                margin = par[1] - par[0]
                faster, slower = dev[1] < par[0] - margin, dev[0] > par[1] + margin
                report.append("  paf2maf, %d x %d: device writer %.3f .. %.3f s, parent %.3f .. %.3f s, parent's spread %.3f s: %s" % (
                    n_rec, mean_ops, dev[0], dev[1], par[0], par[1], margin,
                    "faster beyond the spread" if faster else "slower beyond the spread" if slower else "not shown to be faster or slower"))
            if ok:
                report.append("  outputs equal (%d files against the first): %s" % (compared, same))
                ok = same
            if os.path.exists(first):
                os.remove(first)
            if ok:
                rc, text, err, _ = child([sys.executable, me, "--two-calls", paf], LIMIT_S)
                report.extend(text.strip().split("\n"))
                if rc != 0:
                    report.append("the two calls' step failed (exit %d): %s" % (rc, err.strip()[-300:]))
                    ok = False
            if not ok:
                break
        for p in (paf, t_fa, q_fa):
            if os.path.exists(p):
                os.remove(p)
    text = "\n".join(report) + "\n"
    with open(OUT, "w") as f:
        f.write(text)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
