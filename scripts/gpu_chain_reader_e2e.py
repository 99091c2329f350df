"""The chain reader file to file: `wgatools chain2paf` on a synthetic chain file of N chains with a mean of 30 data lines (a few
hundred MB at the default N), once with the default reader (K23, wga_chain_split; its arrays stay on the device, where K27 writes
the records) and once with WGA_CHAIN_READER=host (the nom-semantics host reader and the host's records, unchanged), both under
WGA_TIMING=1.  One process at a time, each under its own time limit; a step
that fails ends the script.  The two outputs must be equal; both phase lines and wall times go to
profiles/r07_chain_reader_e2e.txt.  Without a visible MI355X the file says so and holds no figure.
Usage: python scripts/gpu_chain_reader_e2e.py [N_CHAINS] [WORKDIR]      (default 1 500 000 chains, a temporary directory)"""
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
OUT = os.path.join(ROOT, "profiles", "r07_chain_reader_e2e.txt")
MEAN_LINES, LIMIT_S = 30, 240


def write_chain_file(path, n_chains, seed=7, piece=50000):
    """chains of 1 .. 59 data lines `size dt dq` (the last one the bare size), consistent with their headers"""
    rng = np.random.default_rng(seed)
    t_size, q_size = 3 * 10 ** 9, 3 * 10 ** 9
    lines_total = 0
    with open(path, "wb") as f:
        for c0 in range(0, n_chains, piece):
            n = min(piece, n_chains - c0)
            nl = rng.integers(1, 2 * MEAN_LINES, n)
            tot = int(nl.sum())
            size = rng.integers(1, 60, tot)
            dt = rng.integers(0, 3, tot) * rng.integers(0, 12, tot)
            dq = rng.integers(0, 3, tot) * rng.integers(0, 12, tot)
            end = np.cumsum(nl)
            dt[end - 1] = 0
            dq[end - 1] = 0
            beg = end - nl
            t_ali = np.add.reduceat(size + dt, beg)
            q_ali = np.add.reduceat(size + dq, beg)
            ts = rng.integers(0, t_size - 10 ** 6, n)
            qs = rng.integers(0, q_size - 10 ** 6, n)
            neg = rng.integers(0, 2, n)
            out = []
            fmt = "%d\t%d\t%d\n".__mod__
            size_l, dt_l, dq_l, beg_l, end_l = size.tolist(), dt.tolist(), dq.tolist(), beg.tolist(), end.tolist()
            ts_l, qs_l, ta_l, qa_l, neg_l = ts.tolist(), qs.tolist(), t_ali.tolist(), q_ali.tolist(), neg.tolist()
            for k in range(n):
                out.append("chain %d chr%d %d + %d %d qchr%d %d %s %d %d %d\n" % (
                    1000 + k, k % 23, t_size, ts_l[k], ts_l[k] + ta_l[k], k % 19, q_size, "-" if neg_l[k] else "+", qs_l[k],
                    qs_l[k] + qa_l[k], c0 + k))
                b, e = beg_l[k], end_l[k]
                out.extend(map(fmt, zip(size_l[b:e - 1], dt_l[b:e - 1], dq_l[b:e - 1])))
                out.append("%d\n\n" % size_l[e - 1])
            f.write("".join(out).encode())
            lines_total += tot
    return lines_total


def main():
    n_chains = int(sys.argv[1]) if len(sys.argv) > 1 else 1500000
    from wgatools_amd import build
    have = False
    if os.path.exists(build.HIP_LIB):
        try:
            import torch  # noqa: F401  first: the library then shares torch's HIP runtime
            have = C.CDLL(build.HIP_LIB).wga_device_count() > 0
        except OSError:
            have = False
    report = []
    if not have or not os.path.exists(build.CLI_BIN):
        report.append("no MI355X visible (or wgatools not built): no figures")
    else:
        work = sys.argv[2] if len(sys.argv) > 2 else tempfile.mkdtemp(prefix="chain_e2e_")
        src = os.path.join(work, "in.chain")
        n_lines = write_chain_file(src, n_chains)
        report.append("chain2paf file to file: %d chains, %d data lines, %.1f MB of chain text" % (
            n_chains, n_lines, os.path.getsize(src) / 1e6))
        outs = []
        for name, env in (("device reader (default)", {}), ("host reader (WGA_CHAIN_READER=host)", {"WGA_CHAIN_READER": "host"})):
            dst = os.path.join(work, "out_%d.paf" % len(outs))
            t0 = time.perf_counter()
            r = subprocess.run(["timeout", "-k", "10", str(LIMIT_S), build.CLI_BIN, "chain2paf", src, "-o", dst, "-r"],
                               env=dict(os.environ, WGA_TIMING="1", **env), stdout=subprocess.PIPE, stderr=subprocess.PIPE)
            wall = time.perf_counter() - t0
            report.append("%s: exit %d, wall %.3f s, %.1f MB of PAF" % (
                name, r.returncode, wall, os.path.getsize(dst) / 1e6 if os.path.exists(dst) else 0.0))
            report.extend("    " + ln for ln in r.stderr.decode(errors="replace").strip().split("\n"))
            if r.returncode != 0:                      # nothing more is started on the device behind a failed step
                report.append("step failed: the run ends here")
                break
            outs.append(dst)
        if len(outs) == 2:
            report.append("outputs equal: %s" % filecmp.cmp(outs[0], outs[1], shallow=False))
        for p in outs + [src]:
            if os.path.exists(p):
                os.remove(p)
    text = "\n".join(report) + "\n"
    with open(OUT, "w") as f:
        f.write(text)
    sys.stdout.write(text)
    return 0 if report and report[-1] == "outputs equal: True" else 1


if __name__ == "__main__":
    sys.exit(main())
