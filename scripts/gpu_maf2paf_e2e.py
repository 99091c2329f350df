"""`maf2paf` file to file at configs[2]'s size: the MAF of scripts/gpu_e2e_at_size.py / gpu_maf_chunk_e2e.py (2 000 000 blocks x
1 500 columns x 2 rows, one copy of 100 000 blocks written 20 times with shifted coordinates; made with numpy here: this process
never opens the GPU), converted three ways: this tree (K28 writes the records: the device writer) three times, the parent commit's
`wgatools` binary five times when WGA_PARENT_CLI names it (the spread of its wall times is the margin: "faster" needs the device
writer's slowest run below the parent's fastest by more than that spread), and this tree with WGA_MAF2PAF_WRITER=host (the
records' fields from host threads, as before K28).  All under WGA_TIMING=1, one process on the GPU at a time (the probe and the
kernel timing are children too), each under its own time limit; the first step that fails ends the script.  The outputs must be
equal byte for byte.  Then both calls of wga_maf2paf alone, in a child process, on the blocks of the file's first GiB (one piece of
the command): the count call and the fill call timed around a synchronise.
Wall times, phase lines and the two calls' bytes and times go to profiles/r07_maf2paf_e2e.txt.  Without a visible MI355X the file
says so and holds no figure.
What to compare: the whole command with the parent's wall times on the same file and box; the fill (bytes written per second)
stands next to the 0.168 TB/s of K27's fill (profiles/r07_chain2paf_e2e.txt) and the 1.33 TB/s of K26's, not against a target.
Usage: python scripts/gpu_maf2paf_e2e.py [COPIES] [WORKDIR]      (default 20 copies of 100 000 blocks, a temporary directory)"""
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
OUT = os.path.join(ROOT, "profiles", "r07_maf2paf_e2e.txt")
LIMIT_S, PARENT_RUNS = 240, 5
NB0, COLS = 100_000, 1500
PIECE = 1 << 30


def child(args, limit, env=None):
    """one process under its own time limit: (exit status, stdout, stderr, wall seconds)"""
    t0 = time.perf_counter()
    r = subprocess.run(["timeout", "-k", "10", str(limit)] + args, env=dict(os.environ, **(env or {})), stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE)
    return r.returncode, r.stdout.decode(errors="replace"), r.stderr.decode(errors="replace"), time.perf_counter() - t0


def write_maf(path, copies):
    """the blocks of gpu_maf_chunk_e2e.py: the query row is the target row, each with a gap in 0.15 % of its columns; every tenth
    block on the `-` strand"""
    rng = np.random.default_rng(3)
    alpha = np.frombuffer(b"ACGT", dtype=np.uint8)
    CH = 20_000
    blocks = []
    for _ in range(0, NB0, CH):
        t = alpha[rng.integers(0, 4, (CH, COLS))]
        q = t.copy()
        q[rng.random((CH, COLS)) < 0.0015] = 45
        t[rng.random((CH, COLS)) < 0.0015] = 45
        blocks.append((t, q))
    with open(path, "wb") as f:
        f.write(b"##maf version=1\n")
        for cp in range(copies):
            for ci, (tn, qn) in enumerate(blocks):
                parts = []
                for k in range(CH):
                    b = cp * NB0 + ci * CH + k
                    parts.append(b"a score=255\ns\tref.chr1\t%d\t1500\t+\t4000000000\t" % (1600 * b))
                    parts.append(tn[k].tobytes())
                    parts.append(b"\ns\tqry.chr1\t%d\t1500\t%s\t4000000000\t" % (1600 * b, b"-" if b % 10 == 0 else b"+"))
                    parts.append(qn[k].tobytes())
                    parts.append(b"\n\n")
                f.write(b"".join(parts))
    return NB0 * copies


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


def two_calls(src, reps=5):
    """a child: the splitter and K3 on the blocks of the file's first GiB, then both calls of wga_maf2paf, each timed"""
    import torch  # noqa: F401
    from wgatools_amd import build, engine, _lib
    eng = engine.Engine(0, _lib.load(build.HIP_LIB))
    with open(src, "rb") as f:
        data = f.read(PIECE)
    data = data[:data.rfind(b"\n\n") + 2]                          # whole blocks
    d_text = eng.upload(np.frombuffer(data + b"\0" * 16, dtype=np.uint8))
    nl = eng.maf_split(d_text, len(data))
    d_lines = eng.empty(nl + 1, engine.MAF_LINE_DTYPE)
    eng.maf_split(d_text, len(data), d_lines)
    lines = d_lines.numpy()[:nl]
    s = lines[lines["status"] == 0]
    t, q = s[0::2], s[1::2]
    n = len(t)
    heads = np.zeros(n, dtype=engine.MAF2PAF_HEAD_DTYPE)
    neg = q["strand_neg"] != 0
    qs, ql, qz = q["num"][:, 0], q["num"][:, 1], q["num"][:, 2]
    heads["q"][:, 0] = qz
    heads["q"][:, 1] = np.where(neg, qz - qs - ql, qs)
    heads["q"][:, 2] = np.where(neg, qz - qs, qs + ql)
    heads["t"][:, 0], heads["t"][:, 1], heads["t"][:, 2] = t["num"][:, 2], t["num"][:, 0], t["num"][:, 0] + t["num"][:, 1]
    heads["strand_neg"] = neg
    for side, ln in (("q", q), ("t", t)):
        heads[side + "name_off"], heads[side + "name_len"] = ln["name_off"], ln["name_len"]
    d_t, d_q = eng.upload(np.ascontiguousarray(t["seq_off"])), eng.upload(np.ascontiguousarray(q["seq_off"]))
    d_c = eng.upload(np.minimum(t["seq_len"], q["seq_len"]))
    d_s = eng.upload(neg.astype(np.uint8))
    counts, run_cnt = eng.maf_pair_stat(n, d_text, d_t, d_q, d_c, d_s)
    run_off = eng.exclusive_scan_u64(n, run_cnt)
    nr = int(run_off.numpy()[-1])
    runs = eng.empty(nr + 1, np.uint64)
    eng.maf_pair_stat(n, d_text, d_t, d_q, d_c, d_s, counts=counts, run_cnt=run_cnt, runs=runs, run_off=run_off)
    d_heads = eng.upload(heads)
    work = eng.empty(int(eng.lib.wga_maf2paf_work_bytes(n, nr)), np.uint8)
    args = (n, d_text, len(data), d_heads, counts, runs, run_off, d_c)
    t_count = []
    for _ in range(reps + 1):                      # the first one warms up
        eng.sync()
        t0 = time.perf_counter()
        total = eng.maf2paf_count(*args, work)
        t_count.append(time.perf_counter() - t0)
    out = eng.empty(total + 16, np.uint8)
    c_total = C.c_uint64(total)
    t_fill = []
    for _ in range(reps + 1):
        eng.sync()
        t0 = time.perf_counter()
        eng._check(eng.lib.wga_maf2paf(eng.ctx, n, d_text.ptr, len(data), d_heads.ptr, counts.ptr, runs.ptr, run_off.ptr, d_c.ptr,
                                       work.ptr, C.byref(c_total), out.ptr))
        eng.sync()
        t_fill.append(time.perf_counter() - t0)
    best = min(t_fill[1:])
    print("both calls of wga_maf2paf: %d blocks, %d runs, %.1f MB of MAF, %.1f MB of PAF out, %.1f MB of workspace" % (
        n, nr, len(data) / 1e6, total / 1e6, int(eng.lib.wga_maf2paf_work_bytes(n, nr)) / 1e6))
    print("    count call %.3f ms best of %d (host clock; plan, scan of %d items, two small copies back)" % (
        min(t_count[1:]) * 1e3, reps, n + nr))
    print("    fill call  %.3f ms best of %d (host clock around a synchronise, one 8-byte copy in front): %.3f TB/s of text written"
          % (best * 1e3, reps, total / best / 1e12))
    eng.close()
    return 0


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--probe":
        return probe()
    if len(sys.argv) > 1 and sys.argv[1] == "--two-calls":
        return two_calls(sys.argv[2])
    copies = int(sys.argv[1]) if len(sys.argv) > 1 else 20
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
        work = sys.argv[2] if len(sys.argv) > 2 else tempfile.mkdtemp(prefix="maf2paf_e2e_")
        src = os.path.join(work, "in.maf")
        t0 = time.perf_counter()
        n_blocks = write_maf(src, copies)
        report.append("maf2paf file to file: %d blocks of %d columns, %.2f GB of MAF (written in %.0f s)" % (
            n_blocks, COLS, os.path.getsize(src) / 1e9, time.perf_counter() - t0))
        parent = os.environ.get("WGA_PARENT_CLI")
        ways = [("this tree (device writer)", build.CLI_BIN, {}, 3)]
        if parent and os.path.exists(parent):
            ways.append(("parent commit's binary", parent, {}, PARENT_RUNS))
        else:
            report.append("WGA_PARENT_CLI not set: the parent commit's binary is NOT measured")
        ways.append(("this tree, WGA_MAF2PAF_WRITER=host", build.CLI_BIN, {"WGA_MAF2PAF_WRITER": "host"}, 1))
        ok = True
        outs, spans = [], {}
        for name, cli, env, runs in ways:
            dst = os.path.join(work, "out_%d.paf" % len(outs))
            walls = []
            for k in range(runs):
                rc, _, err, wall = child([cli, "maf2paf", src, "-o", dst, "-r"], LIMIT_S, dict(env, WGA_TIMING="1"))
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
            report.append("  device writer's slowest %.3f s, parent's fastest %.3f s, parent's spread %.3f s: faster beyond the spread: %s" % (
                dev[1], par[0], margin, dev[1] < par[0] - margin))
        if ok:
            same = all(filecmp.cmp(outs[0], o, shallow=False) for o in outs[1:])
            report.append("  outputs equal (%d files): %s" % (len(outs), same))
            ok = same
        for p in outs:
            if os.path.exists(p):
                os.remove(p)
        if ok:
            rc, text, err, _ = child([sys.executable, me, "--two-calls", src], LIMIT_S)
            report.extend(text.strip().split("\n"))
            if rc != 0:
                report.append("the two calls' step failed (exit %d): %s" % (rc, err.strip()[-300:]))
                ok = False
        if os.path.exists(src):
            os.remove(src)
    text = "\n".join(report) + "\n"
    with open(OUT, "w") as f:
        f.write(text)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
