"""`filter -f paf` file to file: a synthetic PAF of N records with cg:Z: tags of a mean of 5 000 ops (configs[1]'s size at the
default N: about 1.2 GB), filtered with `-b <median span>` and with `-a <median pair sum>` three ways: this tree (K24, the
device path), this tree with WGA_PAF_READER=host (the csv-semantics host path) and, when WGA_PARENT_CLI names it, the parent
commit's `wgatools` binary; all under WGA_TIMING=1, one process at a time, each under its own time limit; a step that fails ends
the script.  The outputs of one setting must be equal byte for byte.  Then the fill kernel alone: both calls of wga_paf_filter
on the first piece of the file in this process, the fill call timed around a synchronise.  Wall times, phase lines and the fill
kernel's bytes and time go to profiles/r07_paf_filter_e2e.txt.  Without a visible MI355X the file says so and holds no figure.
What to compare: the whole command with the parent's wall time on the same file; the fill kernel (bytes read + bytes written
per second) with the 5.85 TB/s of a plain copy.
Usage: python scripts/gpu_paf_filter_e2e.py [N_RECORDS] [WORKDIR]      (default 100 000 records, a temporary directory)"""
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
OUT = os.path.join(ROOT, "profiles", "r07_paf_filter_e2e.txt")
MEAN_OPS, LIMIT_S = 5000, 600


def write_paf_file(path, n, seed=7):
    """records on 40 queries x 25 targets; every cg:Z: is a run of ops out of one random pool.  Returns (median span, median
    pair sum)"""
    rng = np.random.default_rng(seed)
    n_pool = 1 << 22
    lens = rng.integers(1, 2000, n_pool)
    codes = np.frombuffer(b"=XID", dtype=np.uint8)[rng.integers(0, 4, n_pool)]
    ops = [b"%d%c" % (a, c) for a, c in zip(lens.tolist(), codes.tolist())]
    off = np.concatenate([[0], np.cumsum([len(o) for o in ops])])
    pool = b"".join(ops)
    n_ops = rng.integers(1, 2 * MEAN_OPS, n)
    first = rng.integers(0, n_pool - 2 * MEAN_OPS, n)
    ts = rng.integers(0, 10 ** 8, n)
    span = rng.integers(1, 10 ** 6, n)
    q, t = rng.integers(0, 40, n), rng.integers(0, 25, n)
    sums = {}
    with open(path, "wb") as f:
        for k in range(n):
            a, z = int(off[first[k]]), int(off[first[k] + n_ops[k]])
            f.write(b"query%d\t200000000\t%d\t%d\t%s\tchr%d\t150000000\t%d\t%d\t%d\t%d\t60\ttp:A:P\tcg:Z:" % (
                q[k], ts[k], ts[k] + span[k], b"+-"[k & 1:(k & 1) + 1], t[k], ts[k], ts[k] + span[k], span[k] // 2, span[k]))
            f.write(pool[a:z])
            f.write(b"\n")
            sums[(int(q[k]), int(t[k]))] = sums.get((int(q[k]), int(t[k])), 0) + int(span[k])
    return int(np.median(span)), int(np.median(list(sums.values())))


def fill_kernel(src, report, reps=5):
    """both calls of wga_paf_filter on the first piece (at most 1 GiB, cut at a line end), the fill call timed"""
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
    span = d_lines.numpy()[:n]["num"]
    b = int(np.median(span[:, 5] - span[:, 4]))
    par = np.zeros(1, dtype=engine.PAF_FILTER_PARAMS_DTYPE)
    par["min_block_size"] = b
    work = eng.empty(int(eng.lib.wga_paf_filter_work_bytes(n)), np.uint8)
    total, kept, bad = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
    args = (eng.ctx, d_text.ptr, len(data), d_lines.ptr, n, par.ctypes.data, work.ptr, C.byref(total), C.byref(kept), C.byref(bad))
    t0 = time.perf_counter()
    eng._check(eng.lib.wga_paf_filter(*args, None))
    t_count = time.perf_counter() - t0
    out = eng.empty(int(total.value) + 16, np.uint8)
    times = []
    for _ in range(reps + 1):                      # the first one warms up
        eng.sync()
        t0 = time.perf_counter()
        eng._check(eng.lib.wga_paf_filter(*args, out.ptr))
        eng.sync()
        times.append(time.perf_counter() - t0)
    best = min(times[1:])
    report.append("fill kernel on the first piece: %d lines, %.1f MB in, -b %d keeps %d lines, %.1f MB out" % (
        n, len(data) / 1e6, b, kept.value, total.value / 1e6))
    report.append("    count call %.3f ms (host clock, synchronises)" % (t_count * 1e3))
    report.append("    fill call  %.3f ms best of %d (host clock around a synchronise): %.2f TB/s of text written, %.2f TB/s read + written"
                  % (best * 1e3, reps, total.value / best / 1e12, 2 * total.value / best / 1e12))
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
        report.append("no MI355X visible (or wgatools not built): no figures")
    else:
        work = sys.argv[2] if len(sys.argv) > 2 else tempfile.mkdtemp(prefix="paf_filter_e2e_")
        src = os.path.join(work, "in.paf")
        med_span, med_sum = write_paf_file(src, n)
        report.append("filter -f paf file to file: %d records, %.1f MB of PAF" % (n, os.path.getsize(src) / 1e6))
        parent = os.environ.get("WGA_PARENT_CLI")
        ways = [("this tree (device path)", build.CLI_BIN, {}), ("this tree, WGA_PAF_READER=host", build.CLI_BIN, {"WGA_PAF_READER": "host"})]
        if parent and os.path.exists(parent):
            ways.append(("parent commit's binary", parent, {}))
        else:
            report.append("WGA_PARENT_CLI not set: the parent commit's binary is NOT measured")
        ok = True
        for flag, value in (("-b", med_span), ("-a", med_sum)):
            outs = []
            report.append("filter -f paf %s %d" % (flag, value))
            for name, cli, env in ways:
                dst = os.path.join(work, "out_%d.paf" % len(outs))
                t0 = time.perf_counter()
                r = subprocess.run(["timeout", "-k", "10", str(LIMIT_S), cli, "filter", "-f", "paf", flag, str(value), src, "-o", dst, "-r"],
                                   env=dict(os.environ, WGA_TIMING="1", **env), stdout=subprocess.PIPE, stderr=subprocess.PIPE)
                wall = time.perf_counter() - t0
                report.append("  %s: exit %d, wall %.3f s, %.1f MB out" % (
                    name, r.returncode, wall, os.path.getsize(dst) / 1e6 if os.path.exists(dst) else 0.0))
                report.extend("      " + ln for ln in r.stderr.decode(errors="replace").strip().split("\n"))
                if r.returncode != 0:                  # nothing more is started on the device behind a failed step
                    report.append("step failed: the run ends here")
                    ok = False
                    break
                outs.append(dst)
            if not ok:
                break
            same = all(filecmp.cmp(outs[0], o, shallow=False) for o in outs[1:])
            report.append("  outputs equal: %s" % same)
            ok = ok and same
            for p in outs:
                os.remove(p)
        if ok:
            fill_kernel(src, report)
        if os.path.exists(src):
            os.remove(src)
    text = "\n".join(report) + "\n"
    with open(OUT, "w") as f:
        f.write(text)
    sys.stdout.write(text)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
