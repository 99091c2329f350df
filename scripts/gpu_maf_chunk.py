"""K20 (wga_maf_chunk) at size: the count and fill calls' time on device-made blocks, the algorithmic bytes (row bytes read
once + text written once) and their rate against the 8 TB/s peak.  Shapes: configs[2] of gpu_maf_kernels.py (N blocks x
1 500 columns x 2 rows) at -l 100 and -l 1000, 5 N blocks x 300 columns x 2 rows at -l 100, and one block of 10^8 columns x 2 rows at -l 1000000.
Usage: python scripts/gpu_maf_chunk.py [N_BLOCKS [L]]   (default 2 000 000; with L: configs[2] at -l L only, one repetition)"""
import ctypes as C
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from wgatools_amd import _lib, build, engine  # noqa: E402
from wgatools_amd.engine import MAF_CHUNK_BLOCK_DTYPE, MAF_CHUNK_ROW_DTYPE  # noqa: E402


def shape(eng, n_blocks, cols, n_rows=2):
    g = torch.Generator(device="cuda").manual_seed(7)
    alphabet = torch.tensor(list(b"ACGT-"), dtype=torch.uint8, device="cuda")
    nrow = n_blocks * n_rows
    text = alphabet[torch.randint(0, 5, (nrow * cols + 64,), device="cuda", generator=g)]
    text[-64:] = 0
    rows = np.zeros(nrow, dtype=MAF_CHUNK_ROW_DTYPE)
    rows["seq_off"] = np.arange(nrow, dtype=np.uint64) * cols
    rows["seq_len"] = cols
    rows["name_off"] = 0
    rows["name_len"] = 8
    rows["start"] = np.arange(nrow, dtype=np.uint64) * 1000
    rows["src_size"] = 10 ** 9
    return text, eng.upload(rows), nrow


def run(eng, text, d_rows, nrow, n_blocks, n_rows, cols, L, reps=3):
    nk = (cols - 1) // L + 1
    blocks = np.zeros(n_blocks, dtype=MAF_CHUNK_BLOCK_DTYPE)
    blocks["row0"] = np.arange(n_blocks, dtype=np.uint64) * n_rows
    blocks["k_lo"] = 0
    blocks["k_hi"] = nk
    blocks["n_rows"] = n_rows
    n_lines = n_blocks * n_rows * nk
    d_blocks = eng.upload(blocks)
    carry = eng.empty(nrow, np.uint64)
    work = eng.empty(int(eng.lib.wga_maf_chunk_work_bytes(n_blocks, n_lines)), np.uint8)
    total = C.c_uint64(0)
    args = lambda out: (eng.ctx, text.data_ptr(), d_rows.ptr, n_blocks, d_blocks.ptr, n_lines, L, carry.ptr, work.ptr,
                        C.byref(total), out)
    best = None
    out = None
    for _ in range(reps):
        carry.fill(0)
        eng.sync()
        t0 = time.perf_counter()
        eng._check(eng.lib.wga_maf_chunk(*args(None)))
        t1 = time.perf_counter()
        if out is None:
            out = eng.empty(int(total.value) + 16, np.uint8)
        eng._check(eng.lib.wga_maf_chunk(*args(out.ptr)))
        eng.sync()
        t2 = time.perf_counter()
        if best is None or t2 - t0 < best[0] + best[1]:
            best = (t1 - t0, t2 - t1)
    row_bytes = nrow * cols
    alg = row_bytes + int(total.value)
    ms = (best[0] + best[1]) * 1e3
    print("K20 %d blocks x %d cols x %d rows, -l %d: count call %.3f ms, fill call %.3f ms, text %.3f GB; algorithmic %.3f GB "
          "= %.2f TB/s (%.0f %% of 8 TB/s)" % (n_blocks, cols, n_rows, L, best[0] * 1e3, best[1] * 1e3, total.value / 1e9,
                                               alg / 1e9, alg / ms / 1e9, alg / ms / 1e9 / 8 * 100), flush=True)


def main():
    eng = engine.Engine(0, _lib.load(build.HIP_LIB))
    nb = int(sys.argv[1]) if len(sys.argv) > 1 else 2000000
    text, d_rows, nrow = shape(eng, nb, 1500)
    if len(sys.argv) > 2:   # one shape only (the counter passes): configs[2] at -l <argv[2]>
        run(eng, text, d_rows, nrow, nb, 2, 1500, int(sys.argv[2]), reps=1)
        return
    for L in (100, 1000):
        run(eng, text, d_rows, nrow, nb, 2, 1500, L)
    del text
    torch.cuda.empty_cache()
    text, d_rows, nrow = shape(eng, 10 * nb // 2, 300)   # blocks of a few hundred columns: 5 granules per block and row
    run(eng, text, d_rows, nrow, 10 * nb // 2, 2, 300, 100)
    del text
    torch.cuda.empty_cache()
    text, d_rows, nrow = shape(eng, 1, 10 ** 8)
    run(eng, text, d_rows, nrow, 1, 2, 10 ** 8, 1000000)
    eng.close()


if __name__ == "__main__":
    main()
