"""K21 (wga_maf_slice) at size: configs[2]'s blocks (N x 1 500 columns x 2 rows, made on the device), 10^6 regions of 100 to
1 000 bases drawn uniformly on uniformly drawn blocks (anchor = row 0), and K20's `chunk -l 1000` on the same blocks in the
same process.  The passes run under `rocprofv3 --kernel-trace --stats` alone (no counters, no other tracing): this script
starts itself as a fresh child under the profiler, reads the kernel statistics and writes profiles/k21_maf_ext.txt.
Without a visible MI355X the file says so and holds no figure.
Usage: python scripts/gpu_maf_ext.py [N_BLOCKS [N_REGIONS]]      (default 2 000 000 blocks, 1 000 000 regions)"""
import ctypes as C
import csv
import glob
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "profiles", "k21_maf_ext.txt")
COLS, ROWS = 1500, 2


def inner(n_blocks, n_regions):
    import torch
    from wgatools_amd import _lib, build, engine
    from wgatools_amd.engine import MAF_CHUNK_BLOCK_DTYPE, MAF_CHUNK_ROW_DTYPE, MAF_SLICE_HIT_DTYPE, MAF_SLICE_ROW_DTYPE
    eng = engine.Engine(0, _lib.load(build.HIP_LIB))
    g = torch.Generator(device="cuda").manual_seed(7)
    alphabet = torch.tensor(list(b"ACGT-"), dtype=torch.uint8, device="cuda")
    nrow = n_blocks * ROWS
    text = alphabet[torch.randint(0, 5, (nrow * COLS + 64,), device="cuda", generator=g)]
    text[-64:] = 0
    rows = np.zeros(nrow, dtype=MAF_SLICE_ROW_DTYPE)
    rows["seq_off"] = np.arange(nrow, dtype=np.uint64) * COLS
    rows["seq_len"] = COLS
    rows["name_len"] = 8
    rows["start"] = np.arange(nrow, dtype=np.uint64) * 1000
    rows["size"] = 1200
    rows["src_size"] = 10 ** 9
    d_rows = eng.upload(rows)
    rng = np.random.default_rng(11)
    hits = np.zeros(n_regions, dtype=MAF_SLICE_HIT_DTYPE)
    length = rng.integers(100, 1001, n_regions).astype(np.uint64)
    hits["row0"] = rng.integers(0, n_blocks, n_regions).astype(np.uint64) * ROWS
    hits["cut_lo"] = (rng.random(n_regions) * (1200 - length.astype(np.float64)).clip(min=0)).astype(np.uint64)   # a row holds ~1 200 bases
    hits["cut_hi"] = hits["cut_lo"] + length
    hits["n_rows"] = ROWS
    d_hits = eng.upload(hits)
    n_lines, n_cols = n_regions * ROWS, nrow * COLS
    work = eng.empty(int(eng.lib.wga_maf_slice_work_bytes(n_regions, n_lines, nrow, n_cols)), np.uint8)
    total, short = C.c_uint64(0), C.c_uint32(0)
    args = lambda out: (eng.ctx, text.data_ptr(), d_rows.ptr, nrow, n_cols, n_regions, d_hits.ptr, n_lines, work.ptr,
                        C.byref(total), C.byref(short), out)
    out, best = None, None
    for _ in range(3):
        eng.sync()
        t0 = time.perf_counter()
        eng._check(eng.lib.wga_maf_slice(*args(None)))
        t1 = time.perf_counter()
        if out is None:
            out = eng.empty(int(total.value) + 16, np.uint8)
        eng._check(eng.lib.wga_maf_slice(*args(out.ptr)))
        eng.sync()
        t2 = time.perf_counter()
        if best is None or t2 - t0 < sum(best):
            best = (t1 - t0, t2 - t1)
    assert short.value == 0xFFFFFFFF
    print("K21 %d blocks x %d cols x %d rows, %d regions of 100-1000 bases: count call %.3f ms, fill call %.3f ms, text %.3f GB, "
          "table rows %.3f GB" % (n_blocks, COLS, ROWS, n_regions, best[0] * 1e3, best[1] * 1e3, total.value / 1e9, n_cols / 1e9), flush=True)
    print("K21_TEXT_BYTES %d" % total.value)
    del out, work
    # K20 on the same blocks: chunk -l 1000
    crows = np.zeros(nrow, dtype=MAF_CHUNK_ROW_DTYPE)
    for f in ("seq_off", "seq_len", "name_off", "start", "src_size", "name_len", "strand_neg"):
        crows[f] = rows[f]
    d_crows = eng.upload(crows)
    L, nk = 1000, (COLS - 1) // 1000 + 1
    blocks = np.zeros(n_blocks, dtype=MAF_CHUNK_BLOCK_DTYPE)
    blocks["row0"] = np.arange(n_blocks, dtype=np.uint64) * ROWS
    blocks["k_hi"] = nk
    blocks["n_rows"] = ROWS
    d_blocks = eng.upload(blocks)
    carry = eng.empty(nrow, np.uint64)
    cl = n_blocks * ROWS * nk
    cwork = eng.empty(int(eng.lib.wga_maf_chunk_work_bytes(n_blocks, cl)), np.uint8)
    ctotal = C.c_uint64(0)
    cargs = lambda o: (eng.ctx, text.data_ptr(), d_crows.ptr, n_blocks, d_blocks.ptr, cl, L, carry.ptr, cwork.ptr, C.byref(ctotal), o)
    cout, best = None, None
    for _ in range(3):
        carry.fill(0)
        eng.sync()
        t0 = time.perf_counter()
        eng._check(eng.lib.wga_maf_chunk(*cargs(None)))
        t1 = time.perf_counter()
        if cout is None:
            cout = eng.empty(int(ctotal.value) + 16, np.uint8)
        eng._check(eng.lib.wga_maf_chunk(*cargs(cout.ptr)))
        eng.sync()
        t2 = time.perf_counter()
        if best is None or t2 - t0 < sum(best):
            best = (t1 - t0, t2 - t1)
    alg = n_cols + ctotal.value
    print("K20 same blocks, -l 1000: count call %.3f ms, fill call %.3f ms, text %.3f GB; algorithmic %.3f GB = %.2f TB/s"
          % (best[0] * 1e3, best[1] * 1e3, ctotal.value / 1e9, alg / 1e9, alg / sum(best) / 1e12), flush=True)
    print("K20_TEXT_BYTES %d" % ctotal.value)
    eng.close()


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--inner":
        inner(int(sys.argv[2]), int(sys.argv[3]))
        return
    n_blocks = int(sys.argv[1]) if len(sys.argv) > 1 else 2000000
    n_regions = int(sys.argv[2]) if len(sys.argv) > 2 else 1000000
    from wgatools_amd import build
    have = False
    if os.path.exists(build.HIP_LIB):
        try:
            import torch  # noqa: F401  first: the library then shares torch's HIP runtime
            have = C.CDLL(build.HIP_LIB).wga_device_count() > 0
        except OSError:
            have = False
    head = "# K21 (wga_maf_slice), scripts/gpu_maf_ext.py: %d blocks x %d columns x %d rows, %d regions of 100-1000 bases\n" % (
        n_blocks, COLS, ROWS, n_regions)
    if not have:
        open(OUT, "w").write(head + "# NOT RUN: no MI355X was visible where this file was written; K21 has not been measured.\n"
                             "# K20's recorded rate (profiles/k20_maf_chunk.txt, 0.54 TB/s for chunk -l 1000) is the figure to set the fill pass against.\n")
        print("no GPU: wrote", OUT)
        return
    with tempfile.TemporaryDirectory() as tmp:
        r = subprocess.run(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", tmp, "-o", "p", "--",
                            sys.executable, os.path.abspath(__file__), "--inner", str(n_blocks), str(n_regions)],
                           stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=900)
        if r.returncode != 0:
            sys.stderr.write(r.stdout + r.stderr)
            raise SystemExit("the profiled run failed (%d)" % r.returncode)
        stats = {}
        for path in glob.glob(os.path.join(tmp, "**", "*kernel_stats.csv"), recursive=True):
            for row in csv.DictReader(open(path)):
                name = row["Name"].split("(")[0]
                stats[name] = (int(row["Calls"]), float(row["AverageNs"]), float(row["MinNs"]), float(row["MaxNs"]))
    text_bytes = {k: int(v) for k, v in (ln.split() for ln in r.stdout.splitlines() if ln.startswith(("K21_TEXT", "K20_TEXT")))}
    lines = [head, "# host-timed calls (best of 3, same process, under the profiler):\n"]
    lines += ["#   " + ln + "\n" for ln in r.stdout.splitlines() if ln.startswith(("K21 ", "K20 "))]
    lines.append("# rocprofv3 --kernel-trace --stats alone (3 repetitions + nothing else in the process): name calls avg_ns min_ns max_ns\n")
    for name in sorted(stats):
        if "maf_slice" in name or "maf_chunk" in name or "scan" in name:
            lines.append("%s %d %.0f %.0f %.0f\n" % ((name,) + stats[name]))
    n_cols = n_blocks * ROWS * COLS
    for kern, alg, what in (("k_maf_slice_rank", n_cols, "table rows read once"),
                            ("k_maf_slice_fill", 2 * text_bytes.get("K21_TEXT_BYTES", 0), "slices read + text written, about twice the text"),
                            ("k_maf_chunk_fill", n_cols + text_bytes.get("K20_TEXT_BYTES", 0), "rows read + text written")):
        hit = [v for k, v in stats.items() if kern in k]
        if hit:
            lines.append("# %s: %.3f GB (%s) in %.3f ms (min) = %.2f TB/s\n" % (kern, alg / 1e9, what, hit[0][2] / 1e6, alg / hit[0][2] / 1e3))
    open(OUT, "w").write("".join(lines))
    sys.stdout.write("".join(lines))


if __name__ == "__main__":
    main()
