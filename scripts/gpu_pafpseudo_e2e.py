"""`pafpseudo` file to files at the shape of configs[4]'s all-to-all part: 8 genomes of 100 Mb, every genome aligned to every other
one with records of 5 000 ops in the mean (symbol mode: 8 files of 8 rows of 100 MB, 6.4 GB out), made with numpy here (this
process never opens the GPU).  The command is run three ways: this tree (K31 writes the rows' frames in device windows: the device
writer) three times, the parent commit's `wgatools` binary five times when WGA_PARENT_CLI names it (the spread of its wall times is
the margin: "faster" needs the device writer's slowest run below the parent's fastest by more than that spread, and "slower" the
same rule turned round), and this tree with WGA_PSEUDO_WRITER=host (every row a host string, as before K31).  All under
WGA_TIMING=1, one process on the GPU at a time (the probe and the kernel timing are children too), each under its own time limit;
the first step that fails ends the script.  The files of the three ways must be equal byte for byte (compared by a digest of every
file, so that only one way's 6.4 GB stand on the disk at a time).  Base mode needs a FASTA of the 8 genomes: it is run with
`--base`, and the file says so when it was not.  Then both calls of one window alone, in a child process: wga_pafpseudo_fill and
wga_pafpseudo_frame on a window of three 80 MB rows, each timed around a synchronise, with the bytes each wrote.
Wall times, phase lines, the verdict in words and the two calls' bytes and rates go to profiles/r07_pafpseudo_e2e.txt.  Without a
visible MI355X the file says so and holds no figure.
Usage: python scripts/gpu_pafpseudo_e2e.py [--base] [GENOMES] [GENOME_MB] [WORKDIR]   (default 8 genomes of 100 Mb, a temporary
directory)"""
import hashlib
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

OUT = os.path.join(ROOT, "profiles", "r07_pafpseudo_e2e.txt")
LIMIT_S, PARENT_RUNS = 420, 5
MEAN_OPS = 5000
PLAIN_COPY_TBS = 5.85          # the README's figure for a plain device copy


def op_pool(rng, n_pool=1 << 21):
    """a pool of random ops (= X I D, 1 .. 199 long): their text, the text's offsets and the target columns in front of each op"""
    lens = rng.integers(1, 200, n_pool)
    codes = np.frombuffer(b"=XID", dtype=np.uint8)[rng.integers(0, 4, n_pool)]
    ops = [b"%d%c" % (a, c) for a, c in zip(lens.tolist(), codes.tolist())]
    off = np.concatenate([[0], np.cumsum([len(o) for o in ops])])
    cols = np.concatenate([[0], np.cumsum(np.where(codes == ord("I"), 0, lens))])
    bases = np.concatenate([[0], np.cumsum(np.where(codes == ord("D"), 0, lens))])
    return b"".join(ops), off, cols, bases


def write_paf(path, genomes, size, seed=7):
    """every genome against every other one: records that walk along the target with gaps of up to 20 kb and, one time in eight,
    an overlap with the record in front.  Returns the number of records and ops"""
    rng = np.random.default_rng(seed)
    text, off, cols, bases = op_pool(rng)
    n_pool = len(off) - 1
    n_rec = n_ops_all = 0
    with open(path, "wb") as f:
        for q in range(genomes):            # query-major: a target's records are spread over the file
            for t in range(genomes):
                if t == q:
                    continue
                cur = 0
                while True:
                    n_ops = int(rng.integers(1, 2 * MEAN_OPS))
                    first = int(rng.integers(0, n_pool - 2 * MEAN_OPS))
                    span, qspan = int(cols[first + n_ops] - cols[first]), int(bases[first + n_ops] - bases[first])
                    gap = int(rng.integers(0, 20000)) if rng.integers(0, 8) else -int(rng.integers(1, 500))
                    ts = max(0, cur + gap)
                    if ts + span > size or span == 0:
                        break
                    qs = int(rng.integers(0, size - qspan))
                    f.write(b"genome%d\t%d\t%d\t%d\t%s\tgenome%d\t%d\t%d\t%d\t%d\t%d\t60\ttp:A:P\tcg:Z:" % (
                        q, size, qs, qs + qspan, b"+-"[n_rec & 1:(n_rec & 1) + 1], t, size, ts, ts + span, span // 2, span))
                    f.write(text[int(off[first]):int(off[first + n_ops])])
                    f.write(b"\n")
                    cur = max(cur, ts + span)
                    n_rec += 1
                    n_ops_all += n_ops
    return n_rec, n_ops_all


def write_fasta(path, genomes, size, seed=8):
    rng = np.random.default_rng(seed)
    alpha = np.frombuffer(b"ACGT", dtype=np.uint8)
    with open(path, "wb") as f:
        for g in range(genomes):
            f.write(b">genome%d\n" % g)
            seq = alpha[rng.integers(0, 4, size)]
            rows = np.full((size // 100, 101), 10, dtype=np.uint8)       # 100 bases and a newline per line
            rows[:, :100] = seq[:size // 100 * 100].reshape(-1, 100)
            f.write(rows.tobytes())
            if size % 100:
                f.write(seq[size // 100 * 100:].tobytes() + b"\n")


def digest_dir(path):
    """{file: (size, blake2b of its bytes)}"""
    out = {}
    for name in sorted(os.listdir(path)):
        h = hashlib.blake2b(digest_size=16)
        with open(os.path.join(path, name), "rb") as f:
            for piece in iter(lambda: f.read(1 << 24), b""):
                h.update(piece)
        out[name] = (os.path.getsize(os.path.join(path, name)), h.hexdigest())
    return out


def one_window(reps=5):
    """a child: one window of three rows of 80 MB — an `N` row and two query rows of 200 segments with 20 kb of `-` between them —,
    K6's fill call and K31's frame call, each timed around a synchronise"""
    import torch  # noqa: F401
    from wgatools_amd import build, engine, _lib
    eng = engine.Engine(0, _lib.load(build.HIP_LIB))
    rng = np.random.default_rng(3)
    n_rec, row = 400, 80_000_000
    n_ops = rng.integers(MEAN_OPS - 500, MEAN_OPS + 500, n_rec)
    op_off = np.concatenate([[0], np.cumsum(n_ops)]).astype(np.uint64)
    lens = rng.integers(1, 160, int(op_off[-1])).astype(np.uint32)
    codes = np.array([7, 8, 1, 2], dtype=np.uint32)[rng.integers(0, 4, int(op_off[-1]))]     # = X I D
    cols = np.add.reduceat(np.where(codes == 1, 0, lens).astype(np.int64), op_off[:-1].astype(np.int64))
    batch = eng.make_batch(lens << 4 | codes, op_off, np.zeros(n_rec, dtype=np.uint8))
    text = np.frombuffer(b"a score=0\ns\tgenome1\t0\t100000000\t+\t100000000\t", dtype=np.uint8)
    items, dst_off, at = [], np.zeros(n_rec, dtype=np.uint64), 0

    def put(ln, src, kind):
        nonlocal at
        items.append((at, ln, src, kind, 0))
        at += ln
    put(10, 0, engine.SPAN_COPY_TEXT)
    put(len(text) - 10, 10, engine.SPAN_COPY_TEXT)
    put(row, ord("N"), engine.SPAN_FILL)
    put(1, 9, engine.SPAN_COPY_TEXT)
    holes = 0
    for r in range(2):
        put(len(text) - 10, 10, engine.SPAN_COPY_TEXT)
        start = at
        for k in range(r * 200, r * 200 + 200):
            put(20_000, ord("-"), engine.SPAN_FILL)
            dst_off[k] = at
            put(int(cols[k]), 0, engine.SPAN_HOLE)
            holes += int(cols[k])
        put(max(0, row - (at - start)), ord("-"), engine.SPAN_FILL)
        put(1, 9, engine.SPAN_COPY_TEXT)
    total = at
    d_items = eng.upload(np.array(items, dtype=engine.SPAN_ITEM_DTYPE))
    d_text, out = eng.upload(text), eng.empty(total + 64, np.uint8)
    skip, d_dst = eng.upload(np.zeros(n_rec, dtype=np.uint64)), eng.upload(dst_off)
    bad = eng.empty(1, np.uint64)
    t_fill, t_frame = [], []
    for _ in range(reps + 1):                      # the first one warms up
        eng.sync()
        t0 = time.perf_counter()
        eng.pafpseudo_fill(batch, 0, None, 0, None, None, skip, out, d_dst)
        eng.sync()
        t_fill.append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        eng._check(eng.lib.wga_pafpseudo_frame(eng.ctx, len(items), d_items.ptr, None, 0, d_text.ptr, len(text), out.ptr, total, bad.ptr))
        eng.sync()
        t_frame.append(time.perf_counter() - t0)
    assert int(bad.numpy()[0]) == 0xFFFFFFFFFFFFFFFF
    fill, frame = min(t_fill[1:]), min(t_frame[1:])
    print("one window alone: %d items, %.1f MB of text of which %.1f MB are %d segments (%d ops)" % (
        len(items), total / 1e6, holes / 1e6, n_rec, int(op_off[-1])))
    print("    wga_pafpseudo_fill  (K6, symbol mode) %.3f ms best of %d (host clock around a synchronise): %.3f TB/s of segments written"
          % (fill * 1e3, reps, holes / fill / 1e12))
    print("    wga_pafpseudo_frame (K31)             %.3f ms best of %d (host clock around a synchronise): %.3f TB/s of frame written, "
          "next to the %.2f TB/s of a plain copy (which reads what it writes; this kernel only writes)"
          % (frame * 1e3, reps, (total - holes) / frame / 1e12, PLAIN_COPY_TBS))
    print("    peak of device allocations: not recorded (WGA_TIMING does not report it)")
    eng.close()
    return 0


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--probe":
        return probe()
    if len(sys.argv) > 1 and sys.argv[1] == "--one-window":
        return one_window()
    argv = [a for a in sys.argv[1:] if a != "--base"]
    with_base = "--base" in sys.argv[1:]
    genomes = int(argv[0]) if len(argv) > 0 else 8
    size = (int(argv[1]) if len(argv) > 1 else 100) * 1_000_000
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
        work = argv[2] if len(argv) > 2 else tempfile.mkdtemp(prefix="pafpseudo_e2e_")
        parent = os.environ.get("WGA_PARENT_CLI")
        if not (parent and os.path.exists(parent)):
            report.append("WGA_PARENT_CLI not set: the parent commit's binary is NOT measured")
            parent = None
        ok = True
        paf, fa = os.path.join(work, "in.paf"), os.path.join(work, "in.fa")
        t0 = time.perf_counter()
        n_rec, n_ops = write_paf(paf, genomes, size)
        report.append("pafpseudo file to files: %d genomes of %d Mb, all to all: %d records, %d ops (%.0f in the mean), %.2f GB of PAF "
                      "(written in %.0f s)" % (genomes, size // 1_000_000, n_rec, n_ops, n_ops / max(n_rec, 1), os.path.getsize(paf) / 1e9,
                                               time.perf_counter() - t0))
        modes = [("symbol mode", [])]
        if with_base:
            t0 = time.perf_counter()
            write_fasta(fa, genomes, size)
            report.append("base mode: %.2f GB of FASTA (written in %.0f s)" % (os.path.getsize(fa) / 1e9, time.perf_counter() - t0))
            modes.append(("base mode", ["-f", fa]))
        else:
            report.append("base mode was NOT run (it needs --base and the time to write and read 0.8 GB of FASTA)")
        for mode, extra in modes:
            ways = [("this tree (device writer)", build.CLI_BIN, {}, 3)]
            if parent:
                ways.append(("parent commit's binary", parent, {}, PARENT_RUNS))
            ways.append(("this tree, WGA_PSEUDO_WRITER=host", build.CLI_BIN, {"WGA_PSEUDO_WRITER": "host"}, 1))
            digests, spans = [], {}
            for name, cli, env, runs in ways:
                dst = os.path.join(work, "out")
                walls = []
                for k in range(runs):
                    rc, _, err, wall = child([cli, "pafpseudo", paf, "-o", dst, "-r"] + extra, LIMIT_S, dict(env, WGA_TIMING="1"))
                    walls.append(wall)
                    size_out = sum(os.path.getsize(os.path.join(dst, f)) for f in os.listdir(dst)) if os.path.isdir(dst) else 0
                    report.append("  %s, %s%s: exit %d, wall %.3f s, %.1f MB out" % (
                        mode, name, " (run %d)" % (k + 1) if runs > 1 else "", rc, wall, size_out / 1e6))
                    report.extend("      " + ln for ln in err.strip().split("\n"))
                    if rc != 0:                            # nothing more is started on the device behind a failed step
                        report.append("step failed: the run ends here")
                        ok = False
                        break
                if not ok:
                    break
                if runs > 1:
                    report.append("  %s, %s: wall min %.3f s, median %.3f s, max %.3f s over %d runs" % (
                        mode, name, min(walls), float(np.median(walls)), max(walls), runs))
                    spans[cli] = (min(walls), max(walls))
                digests.append(digest_dir(dst))
                shutil.rmtree(dst)
            if ok and parent in spans:
                dev, par = spans[build.CLI_BIN], spans[parent]
                margin = par[1] - par[0]
                faster, slower = dev[1] < par[0] - margin, dev[0] > par[1] + margin
                report.append("  %s: device writer %.3f .. %.3f s, parent %.3f .. %.3f s, parent's spread %.3f s" % (
                    mode, dev[0], dev[1], par[0], par[1], margin))
                report.append("  verdict, %s: the device writer is %s" % (
                    mode, "FASTER than the parent beyond the parent's spread" if faster else
                    "SLOWER than the parent beyond the parent's spread" if slower else
                    "NOT shown to be faster or slower than the parent (the difference lies inside the parent's spread)"))
            elif ok:
                report.append("  verdict, %s: none (the parent commit's binary was not measured)" % mode)
            if ok:
                same = all(d == digests[0] for d in digests[1:])
                report.append("  %s: files equal over the %d ways (%d files, %.2f GB): %s" % (
                    mode, len(digests), len(digests[0]), sum(v[0] for v in digests[0].values()) / 1e9, same))
                ok = same
            if not ok:
                break
        if ok:
            rc, text, err, _ = child([sys.executable, me, "--one-window"], LIMIT_S)
            report.extend(text.strip().split("\n"))
            if rc != 0:
                report.append("the one window's step failed (exit %d): %s" % (rc, err.strip()[-300:]))
                ok = False
        for p in (paf, fa):
            if os.path.exists(p):
                os.remove(p)
    text = "\n".join(report) + "\n"
    with open(OUT, "w") as f:
        f.write(text)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
