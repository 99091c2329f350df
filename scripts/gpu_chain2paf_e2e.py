"""`chain2paf` file to file: the synthetic chain file of scripts/gpu_chain_reader_e2e.py (N chains with a mean of 30 data lines, a
few hundred MB at the default N), converted four ways: this tree (K23 reads, K27 writes: the device path) three times, the parent
commit's `wgatools` binary five times when WGA_PARENT_CLI names it (the spread of its wall times is the margin: "faster" needs
the device path's slowest run below the parent's fastest by more than that spread), this tree with WGA_CHAIN2PAF_WRITER=host (the
device reader, the host's records) and this tree with WGA_CHAIN_READER=host (the host reader, the host's records).  All under
WGA_TIMING=1, one process on the GPU at a time (this process itself never opens it: the probe and the kernel timing are children
too), each under its own time limit; the first step that fails ends the script.  The outputs must be equal byte for byte.  Then
the fill kernel alone, in a child process: both calls of wga_chain2paf on the file, the fill call timed around a synchronise.
Wall times, phase lines and the fill call's bytes and time go to profiles/r07_chain2paf_e2e.txt.  Without a visible MI355X the
file says so and holds no figure.
What to compare: the whole command with the parent's wall times on the same file and box; the fill kernel (bytes written per
second) with the 0.145 TB/s of K25's fill (profiles/r07_chain_filter_e2e.txt).
Usage: python scripts/gpu_chain2paf_e2e.py [N_CHAINS] [WORKDIR]      (default 1 500 000 chains, a temporary directory)"""
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
OUT = os.path.join(ROOT, "profiles", "r07_chain2paf_e2e.txt")
LIMIT_S, PARENT_RUNS = 240, 5


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
    """a child: K23 on the file, then both calls of wga_chain2paf, the fill call timed"""
    import torch  # noqa: F401
    from wgatools_amd import build, engine, _lib
    eng = engine.Engine(0, _lib.load(build.HIP_LIB))
    with open(src, "rb") as f:
        data = f.read()
    d_text = eng.upload(np.frombuffer(data + b"\0" * 16, dtype=np.uint8))
    nc, nd, st, bad = eng.chain_split(d_text, len(data))
    heads, lines, off = eng.empty(nc + 1, engine.CHAIN_HEAD_DTYPE), eng.empty((nd + 1) * 3, np.uint64), eng.empty(nc + 1, np.uint64)
    eng.chain_split(d_text, len(data), heads, lines, off)
    work = eng.empty(int(eng.lib.wga_chain2paf_work_bytes(nc, nd)), np.uint8)
    eng.sync()
    t0 = time.perf_counter()
    total = eng.chain2paf_count(d_text, len(data), heads, nc, lines, off, work)
    t_count = time.perf_counter() - t0
    out = eng.empty(total + 16, np.uint8)
    c_total = C.c_uint64(total)
    times = []
    for _ in range(reps + 1):                      # the first one warms up
        eng.sync()
        t0 = time.perf_counter()
        eng._check(eng.lib.wga_chain2paf(eng.ctx, d_text.ptr, len(data), heads.ptr, nc, lines.ptr, off.ptr, work.ptr, C.byref(c_total),
                                         out.ptr))
        eng.sync()
        times.append(time.perf_counter() - t0)
    best = min(times[1:])
    print("fill kernel: %d chains, %d data lines, %.1f MB in, %.1f MB of PAF out, %.1f MB of workspace" % (
        nc, nd, len(data) / 1e6, total / 1e6, int(eng.lib.wga_chain2paf_work_bytes(nc, nd)) / 1e6))
    print("    count call %.3f ms (host clock; two scans of %d lines, plan, scan of %d items, two small copies back)" % (
        t_count * 1e3, nd, nc + nd))
    print("    fill call  %.3f ms best of %d (host clock around a synchronise, one 8-byte copy in front): %.3f TB/s of text written"
          % (best * 1e3, reps, total / best / 1e12))
    eng.close()
    return 0


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--probe":
        return probe()
    if len(sys.argv) > 1 and sys.argv[1] == "--fill-kernel":
        return fill_kernel(sys.argv[2])
    n_chains = int(sys.argv[1]) if len(sys.argv) > 1 else 1500000
    from wgatools_amd import build
    from gpu_chain_reader_e2e import write_chain_file
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
        work = sys.argv[2] if len(sys.argv) > 2 else tempfile.mkdtemp(prefix="chain2paf_e2e_")
        src = os.path.join(work, "in.chain")
        n_lines = write_chain_file(src, n_chains)
        report.append("chain2paf file to file: %d chains, %d data lines, %.1f MB of chain text" % (
            n_chains, n_lines, os.path.getsize(src) / 1e6))
        parent = os.environ.get("WGA_PARENT_CLI")
        ways = [("this tree (device reader, device writer)", build.CLI_BIN, {}, 3)]
        if parent and os.path.exists(parent):
            ways.append(("parent commit's binary", parent, {}, PARENT_RUNS))
        else:
            report.append("WGA_PARENT_CLI not set: the parent commit's binary is NOT measured")
        ways += [("this tree, WGA_CHAIN2PAF_WRITER=host", build.CLI_BIN, {"WGA_CHAIN2PAF_WRITER": "host"}, 1),
                 ("this tree, WGA_CHAIN_READER=host", build.CLI_BIN, {"WGA_CHAIN_READER": "host"}, 1)]
        ok = True
        outs, spans = [], {}
        for name, cli, env, runs in ways:
            dst = os.path.join(work, "out_%d.paf" % len(outs))
            walls = []
            for k in range(runs):
                rc, _, err, wall = child([cli, "chain2paf", src, "-o", dst, "-r"], LIMIT_S, dict(env, WGA_TIMING="1"))
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
            report.append("  device path's slowest %.3f s, parent's fastest %.3f s, parent's spread %.3f s: faster beyond the spread: %s" % (
                dev[1], par[0], margin, dev[1] < par[0] - margin))
        if ok:
            same = all(filecmp.cmp(outs[0], o, shallow=False) for o in outs[1:])
            report.append("  outputs equal (%d files): %s" % (len(outs), same))
            ok = same
        for p in outs:
            if os.path.exists(p):
                os.remove(p)
        if ok:
            rc, text, err, _ = child([sys.executable, me, "--fill-kernel", src], LIMIT_S)
            report.extend(text.strip().split("\n"))
            if rc != 0:
                report.append("fill kernel step failed (exit %d): %s" % (rc, err.strip()[-300:]))
                ok = False
        if os.path.exists(src):
            os.remove(src)
    text = "\n".join(report) + "\n"
    with open(OUT, "w") as f:
        f.write(text)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
