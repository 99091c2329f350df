"""File to file at configs[2]'s size: `wgatools chunk -l 1000` next to `wgatools maf2paf` on the same MAF (2 000 000 blocks x
1 500 columns x 2 rows, written as scripts/gpu_e2e_at_size.py writes it), wall time and the WGA_TIMING=1 phases.
Usage: python scripts/gpu_maf_chunk_e2e.py [TMPDIR]"""
import os
import subprocess
import sys
import tempfile
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "wgatools_amd", "bin", "wgatools")
tmp = sys.argv[1] if len(sys.argv) > 1 else tempfile.mkdtemp()
nb0, cols, copies = 100_000, 1500, 20
dev = torch.device("cuda", 0)
g = torch.Generator(device=dev)
g.manual_seed(3)
alpha = torch.tensor(list(b"ACGT"), dtype=torch.uint8, device=dev)
maf = os.path.join(tmp, "in.maf")
t0 = time.perf_counter()
CH = 20_000
blocks = []
for c0 in range(0, nb0, CH):   # one copy of 100 000 blocks, written 20 times with shifted coordinates
    t = alpha[torch.randint(0, 4, (CH, cols), device=dev, generator=g)]
    q = t.clone()
    q[torch.rand((CH, cols), device=dev, generator=g) < 0.0015] = 45
    t[torch.rand((CH, cols), device=dev, generator=g) < 0.0015] = 45
    blocks.append((t.cpu().numpy(), q.cpu().numpy()))
with open(maf, "wb") as f:
    f.write(b"##maf version=1\n")
    for cp in range(copies):
        for ci, (tn, qn) in enumerate(blocks):
            parts = []
            for k in range(CH):
                b = cp * nb0 + ci * CH + k
                parts.append(b"a score=255\ns\tref.chr1\t%d\t1500\t+\t4000000000\t" % (1600 * b))
                parts.append(tn[k].tobytes())
                parts.append(b"\ns\tqry.chr1\t%d\t1500\t%s\t4000000000\t" % (1600 * b, b"-" if b % 10 == 0 else b"+"))
                parts.append(qn[k].tobytes())
                parts.append(b"\n\n")
            f.write(b"".join(parts))
print("MAF: %d blocks, %.2f GB, written in %.0f s" % (nb0 * copies, os.path.getsize(maf) / 1e9, time.perf_counter() - t0),
      flush=True)
for name, args in (("maf2paf", ["maf2paf", maf]), ("chunk -l 1000", ["chunk", maf, "-l", "1000"]),
                   ("chunk -l 1000", ["chunk", maf, "-l", "1000"]), ("maf2paf", ["maf2paf", maf])):
    out = os.path.join(tmp, "out.txt")
    t0 = time.perf_counter()
    r = subprocess.run([CLI, "-r", "-o", out] + args, stderr=subprocess.PIPE, env=dict(os.environ, WGA_TIMING="1"))
    dt = time.perf_counter() - t0
    ph = [l for l in r.stderr.decode().splitlines() if "timing" in l]
    print("%-14s rc=%d %.2f s, output %.2f GB\n    %s" % (name, r.returncode, dt, os.path.getsize(out) / 1e9 if os.path.exists(out) else 0,
                                                      "\n    ".join(ph) or r.stderr.decode()[-300:]), flush=True)
    if os.path.exists(out):
        os.remove(out)
os.remove(maf)
