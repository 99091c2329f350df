"""K22 (wga_maf_rewrite) at size: configs[2]'s blocks (N x 1 500 columns x 2 rows, made on the device) rewritten whole (the
`rename` case with two prefixes, and the `filter` case with thresholds that drop about half of the blocks), and on the same
blocks in the same process what the parent of K22 offered for this job: K21 (wga_maf_slice) with every hit `whole`.
Host-timed calls (the count call holds its read-back), one warm-up, then REPS repetitions each into a fresh output buffer;
the medians go to profiles/k22_maf_rewrite.txt.  Without a visible MI355X the file says so and holds no figure.
Usage: python scripts/gpu_maf_rewrite.py [N_BLOCKS]      (default 2 000 000 blocks)"""
import ctypes as C
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "profiles", "k22_maf_rewrite.txt")
COLS, ROWS, REPS = 1500, 2, 5


def timed(eng, call, text_bytes):
    """call(out_ptr_or_None) twice per repetition (count, fill); (median count s, median fill s, median of their sums)"""
    cnt, fill = [], []
    for rep in range(REPS + 1):
        eng.sync()
        t0 = time.perf_counter()
        call(None)
        t1 = time.perf_counter()
        out = eng.empty(int(text_bytes()) + 16, np.uint8)      # a fresh buffer: its pages are first touched by the fill
        eng.sync()
        t2 = time.perf_counter()
        call(out.ptr)
        eng.sync()
        t3 = time.perf_counter()
        del out
        if rep:                                                  # the first repetition is the warm-up
            cnt.append(t1 - t0)
            fill.append(t3 - t2)
    return statistics.median(cnt), statistics.median(fill), statistics.median([a + b for a, b in zip(cnt, fill)])


def main():
    n_blocks = int(sys.argv[1]) if len(sys.argv) > 1 else 2000000
    from wgatools_amd import build
    have = False
    if os.path.exists(build.HIP_LIB):
        try:
            import torch  # noqa: F401  first: the library then shares torch's HIP runtime
            have = C.CDLL(build.HIP_LIB).wga_device_count() > 0
        except OSError:
            have = False
    head = "# K22 (wga_maf_rewrite), scripts/gpu_maf_rewrite.py: %d blocks x %d columns x %d rows\n" % (n_blocks, COLS, ROWS)
    if not have:
        open(OUT, "w").write(head + "# NOT RUN: no MI355X was visible where this file was written; K22 has not been measured, and neither\n"
                             "# has K21 with every hit `whole` on the same blocks.\n")
        print("no GPU: wrote", OUT)
        return
    import torch
    from wgatools_amd import _lib, engine
    from wgatools_amd.engine import MAF_REWRITE_BLOCK_DTYPE, MAF_REWRITE_PARAMS_DTYPE, MAF_SLICE_HIT_DTYPE, MAF_SLICE_ROW_DTYPE
    eng = engine.Engine(0, _lib.load(build.HIP_LIB))
    g = torch.Generator(device="cuda").manual_seed(7)
    alphabet = torch.tensor(list(b"ACGT-"), dtype=torch.uint8, device="cuda")
    nrow = n_blocks * ROWS
    text = alphabet[torch.randint(0, 5, (nrow * COLS + 64,), device="cuda", generator=g)]
    text[-64:] = 0
    rng = np.random.default_rng(11)
    rows = np.zeros(nrow, dtype=MAF_SLICE_ROW_DTYPE)
    rows["seq_off"] = np.arange(nrow, dtype=np.uint64) * COLS
    rows["seq_len"] = COLS
    rows["name_len"] = 8
    rows["start"] = np.arange(nrow, dtype=np.uint64) * 1000
    rows["size"] = rng.integers(1000, 1400, nrow).astype(np.uint64)
    rows["src_size"] = 10 ** 9
    d_rows = eng.upload(rows)
    blocks = np.zeros(n_blocks, dtype=MAF_REWRITE_BLOCK_DTYPE)
    blocks["row0"] = np.arange(n_blocks, dtype=np.uint64) * ROWS
    blocks["n_rows"] = ROWS
    d_blocks = eng.upload(blocks)
    n_lines, n_cols = nrow, nrow * COLS
    d_ptext = eng.upload(np.frombuffer(b"hg38.mm39." + b"\0" * 16, dtype=np.uint8))
    d_poff = eng.upload(np.array([0, 5, 10], dtype=np.uint32))
    work = eng.empty(int(eng.lib.wga_maf_rewrite_work_bytes(n_blocks, n_lines)), np.uint8)
    lines = [head, "# host-timed calls, medians of %d repetitions behind one warm-up, a fresh output buffer each; the count call holds its read-back\n" % REPS]
    results = {}
    for label, filt, npre in (("rename, 2 prefixes of 5 bytes", 0, 2), ("filter -b 1200 (about half of the blocks)", 1, 0), ("every block, no prefix", 0, 0)):
        par = np.zeros(1, dtype=MAF_REWRITE_PARAMS_DTYPE)
        par["filter"], par["min_block_size"], par["n_prefix"] = filt, 1200, npre
        par["d_prefix_text"], par["d_prefix_off"] = d_ptext.ptr, d_poff.ptr
        total, kept, bad = C.c_uint64(0), C.c_uint32(0), C.c_uint32(0)

        def call(out):
            eng._check(eng.lib.wga_maf_rewrite(eng.ctx, text.data_ptr(), d_rows.ptr, n_blocks, d_blocks.ptr, n_lines, par.ctypes.data,
                                               work.ptr, C.byref(total), C.byref(kept), C.byref(bad), out))
        c, f, s = timed(eng, call, lambda: total.value)
        assert bad.value == 0xFFFFFFFF
        rows_in = int(kept.value) * ROWS * COLS
        results[label] = (c, f, s, total.value)
        lines.append("K22 %s: kept %d blocks, count call %.3f ms, fill call %.3f ms, both %.3f ms; text %.3f GB, kept rows %.3f GB; "
                     "fill = %.2f TB/s of rows in + text out\n" % (label, kept.value, c * 1e3, f * 1e3, s * 1e3, total.value / 1e9, rows_in / 1e9,
                                                                    (rows_in + total.value) / f / 1e12))
    del work
    hits = np.zeros(n_blocks, dtype=MAF_SLICE_HIT_DTYPE)
    hits["row0"] = blocks["row0"]
    hits["n_rows"] = ROWS
    hits["whole"] = 1
    d_hits = eng.upload(hits)
    swork = eng.empty(int(eng.lib.wga_maf_slice_work_bytes(n_blocks, n_lines, nrow, n_cols)), np.uint8)
    stotal, short = C.c_uint64(0), C.c_uint32(0)

    def scall(out):
        eng._check(eng.lib.wga_maf_slice(eng.ctx, text.data_ptr(), d_rows.ptr, nrow, n_cols, n_blocks, d_hits.ptr, n_lines, swork.ptr,
                                         C.byref(stotal), C.byref(short), out))
    c, f, s = timed(eng, scall, lambda: stotal.value)
    lines.append("K21 every hit whole, same blocks: count call %.3f ms, fill call %.3f ms, both %.3f ms; text %.3f GB\n"
                 % (c * 1e3, f * 1e3, s * 1e3, stotal.value / 1e9))
    k22 = results["every block, no prefix"]
    assert k22[3] == stotal.value
    lines.append("# the same text both ways (%d bytes): K22 count + fill %.3f ms against K21's %.3f ms\n" % (stotal.value, k22[2] * 1e3, s * 1e3))
    open(OUT, "w").write("".join(lines))
    sys.stdout.write("".join(lines))
    eng.close()


if __name__ == "__main__":
    main()
