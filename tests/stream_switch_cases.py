"""Record switches, tile borders and stream restarts of the streaming row kernel (expand_variant 3 / pseudo_variant 3), written
once and run twice: tests/test_emu_stream_switch.py on the SIMT emulator, tests/test_gpu_stream_switch.py on an MI355X.

The kernel reads a job's skip word, the next record's end and fields and a tile's descriptor as wave-uniform scalar reads; these
batches put a switch, a border or a restart at every place where one of those reads decides what happens next:
  * records of 1, 2, 255, 256, 257, 1 023, 1 024 and 1 025 ops, laid out so that records end exactly on an intake border (256
    ops), a tile border (1 024) and a job border; several one-op records in a row (switches with no super-step between them);
  * records without ops: first and last in the batch, alone, in runs of three, on a tile border, behind a record that ends on
    a job border;
  * tiles left to v1 — the first and the last tile of a job, a whole job, two adjacent whole jobs, the batch's last tile — each
    between clean tiles of long records, so that the stream stops and starts again inside a record.  What leaves them: a query
    slice one byte longer or one byte shorter than the CIGAR consumes, a slice within 32 bytes of either pool edge;
  * both strands, an invalid base in a '-' record that begins behind a switch.
Batches are three to five jobs long (plus a partial tile, so that the tile count is no multiple of the job size).
Every comparison is equality of bytes / integers: variant 3 against variant 0 over the whole pre-filled output buffer and the
diagnostics, the rows against the oracle (parity_cases.check_paf2maf), bytes outside the rows and the canary keep the fill."""
import numpy as np

import oracle_py as orc
import parity_cases as pc

NONE = pc.NONE

TILE = 1024
FILL = 0x23
JOB_TILES = (1, 2, 4, 8, 32)
EQ, X, I, D = 7, 8, 1, 2


# ---- batches ------------------------------------------------------------------------------------------------------------
class _Builder:
    """records as op counts; `kind` says what the slices look like: 0 clean, 'long' / 'short' a query slice one byte longer /
    shorter than the CIGAR consumes, 'head' / 'tail' a query slice within 32 bytes of the pool's start / end"""

    def __init__(self, seed):
        self.rng = np.random.default_rng(seed)
        self.n_ops, self.kind, self.bad = [], [], []
        self.p = 0

    def rec(self, n_ops, kind=0, bad=False):
        self.n_ops.append(int(n_ops))
        self.kind.append(kind)
        self.bad.append(bad)
        self.p += int(n_ops)

    def empty(self, k=1):
        for _ in range(k):
            self.rec(0)

    def to(self, target, kind=0):
        """one record that ends exactly at op `target`"""
        assert target > self.p, (target, self.p)
        self.rec(target - self.p, kind)

    def ops_of(self, n):
        """= runs with an edit between them; one- and two-op records are an = run (and an insertion)"""
        rng = self.rng
        code = np.where(np.arange(n) % 2 == 0, EQ, rng.choice(np.array([X, I, D], dtype=np.uint32), n, p=[0.4, 0.3, 0.3]))
        if n % 2 == 0 and n > 2:
            code[-1] = EQ       # a record ends with an = run (two = runs in a row are fine)
        ln = np.where(code == EQ, rng.integers(1, 10, n), rng.integers(1, 4, n))
        ln = np.where((code != EQ) & (rng.random(n) < 0.004), rng.integers(40, 300, n), ln)     # a long gap now and then
        return (ln.astype(np.uint32) << np.uint32(4)) | code.astype(np.uint32)

    def build(self, strands=None):
        rng = self.rng
        n = len(self.n_ops)
        ops = [self.ops_of(k) for k in self.n_ops]
        op_off = np.zeros(n + 1, dtype=np.uint64)
        op_off[1:] = np.cumsum(self.n_ops)
        strand = rng.integers(0, 2, n).astype(np.uint8) if strands is None else np.asarray(strands, dtype=np.uint8)
        t_len, q_len = np.zeros(n, dtype=np.uint64), np.zeros(n, dtype=np.uint64)
        for i, o in enumerate(ops):
            code, ln = o & 15, (o >> 4).astype(np.int64)
            t_len[i] = int(ln[(code == EQ) | (code == X) | (code == D)].sum())
            q_len[i] = int(ln[(code == EQ) | (code == X) | (code == I)].sum())
            if self.bad[i]:
                strand[i] = 1
        for i, k in enumerate(self.kind):
            if k == "long":
                q_len[i] += 1
            elif k == "short":
                q_len[i] -= 1
        # pools: 64 bytes of padding around the slices, but the 'head' / 'tail' records' query slices lie 8 bytes from the pool's
        # edges (the first 'head' and the last 'tail' record; further ones are ordinary, still one byte off clean: 'long')
        heads = [i for i, k in enumerate(self.kind) if k == "head"]
        tails = [i for i, k in enumerate(self.kind) if k == "tail"]
        for i in heads[1:] + tails[:-1]:
            q_len[i] += 1
        order = heads[:1] + [i for i in range(n) if i not in heads[:1] + tails[-1:]] + tails[-1:]
        q_off = np.zeros(n, dtype=np.uint64)
        pos = 8 if heads else 64
        for j, i in enumerate(order):
            if j == 1 and heads:
                pos += 64
            if tails and i == tails[-1]:
                pos += 64
            q_off[i] = pos
            pos += int(q_len[i])
        q_bytes = pos + (8 if tails else 64)
        t_off = np.zeros(n, dtype=np.uint64)
        t_off[1:] = np.cumsum(t_len)[:-1]
        t_off += np.uint64(64)
        t_bytes = 64 + int(t_len.sum()) + 64
        lut = np.frombuffer(b"ACGTacgtNn", dtype=np.uint8)
        t_pool = lut[rng.integers(0, len(lut), t_bytes)]
        q_pool = lut[rng.integers(0, len(lut), q_bytes)]
        for i in range(n):
            if self.bad[i]:      # an invalid base two thirds into a '-' record, in an = run (pafpseudo never reads inserted bases)
                code, ln = ops[i] & 15, (ops[i] >> 4).astype(np.int64)
                k = (2 * len(code) // 3) & ~1
                idx = int(ln[:k][(code[:k] == EQ) | (code[:k] == X) | (code[:k] == I)].sum())
                q_pool[int(q_off[i]) + int(q_len[i]) - 1 - idx] = ord("R")
        return dict(ops=np.concatenate(ops).astype(np.uint32) if self.p else np.zeros(0, np.uint32), op_off=op_off,
                    strand_neg=strand, t_pool=t_pool, q_pool=q_pool, t_src_off=t_off, q_src_off=q_off, t_src_len=t_len,
                    q_src_len=q_len)


def lengths_batch(jt, seed=1):
    """the record lengths and the records without ops; nothing is left to v1.  Three jobs and a partial tile."""
    job = jt * TILE
    b = _Builder(seed * 100 + jt)
    b.empty()                               # first in the batch
    for k in (1, 1, 1, 2, 1):
        b.rec(k)                            # switches with no super-step between them
    b.to(256)                               # ends on an intake border
    for k in (255, 256, 257):               # 256 + 768: the last one ends on the tile border at op 1 024
        b.rec(k)
    b.empty(3)                              # a run of three on a tile border
    b.rec(1023)
    b.rec(1)                                # ends on the tile border at 2 048
    b.rec(1024)
    b.empty()                               # alone, on a tile border
    b.rec(1025, bad=True)                   # '-' strand with an invalid base: begins behind a switch, ends one op into a tile
    b.rec(2)
    b.rec(255)
    nxt = (b.p // job + 1) * job
    b.to(nxt)                               # ends on a job border ...
    b.empty()                               # ... with a record without ops directly behind it
    b.rec(1)
    b.empty(3)
    b.rec(257)
    end = max(3 * job, nxt + job) + 300
    b.to(end - 1)                           # a long record over the rest (whole jobs for the longer job sizes)
    b.rec(1)
    b.empty()                               # last in the batch
    return b.build()


def skip_batch(jt, which, seed=2):
    """tiles left to v1 inside long clean records.  which = 'edges': the first tile of job 1, the last tile of job 2 and the
    batch's last tile; 'job': all of job 1; 'jobs': all of jobs 1 and 2"""
    job = jt * TILE
    b = _Builder(seed * 100 + jt + {"edges": 0, "job": 1000, "jobs": 2000}[which])
    kinds = ["long", "short", "head", "tail"]

    def mark(tile, kind):
        """a two-op record that is not the streaming kernel's, in the middle of `tile`; long clean records around it"""
        b.to(tile * TILE + 500)
        b.rec(2, kind)

    b.rec(3)
    if which == "edges":
        n_jobs = 4
        mark(jt, kinds[0])                   # first tile of job 1
        mark(3 * jt - 1, kinds[1])           # last tile of job 2
        last = n_jobs * jt                   # the partial tile behind the last whole job
        b.to(last * TILE + 100)
        b.rec(2, kinds[2])
        b.rec(1, kinds[3])
        b.to(last * TILE + 300)
    else:
        n_jobs = 4 if which == "job" else 5
        lo, hi = job, (2 if which == "job" else 3) * job
        b.to(lo + 7)                         # clean: ends inside the first skipped tile
        b.to(hi - 9, kinds[(jt + (which == "jobs")) % 4])     # one record that is not clean over every tile of the job(s)
        b.rec(1)
        b.to(n_jobs * job + 300)             # clean from inside the last skipped tile to the end
    return b.build()


def all_batches(jt):
    yield "lengths", lengths_batch(jt)
    for which in ("edges", "job", "jobs"):
        yield which, skip_batch(jt, which)


# ---- checks -------------------------------------------------------------------------------------------------------------
def _n_tiles(b):
    return (len(b["ops"]) + TILE - 1) // TILE


def _with_ops(b):
    """the records the oracle is asked about: the reference rejects an empty CIGAR when it parses the line, before any row code
    runs, so a record without ops has no rows to compare (its rows have no bytes and it raises no diagnostic here)"""
    return [int(i) for i in np.flatnonzero(b["op_off"][1:] > b["op_off"][:-1])]


def check_paf2maf_batch(eng, b, jt, expect_left):
    """variant 3 == variant 0 over the whole buffer and the diagnostics; every record against the oracle; fill and canary"""
    before = eng.get_param("expand_job_tiles")
    eng.set_param("expand_job_tiles", jt)
    recs = _with_ops(b)
    try:
        r3 = pc.check_paf2maf(eng, b, variant=3, sample=recs)
        assert eng.get_param("expand_variant_used") == 3
        left = eng.get_param("expand_stream_left_to_v1")
        r0 = pc.run_paf2maf(eng, b, variant=0)
        rs = pc.check_paf2maf(eng, b, force_slow=1, variant=3, sample=recs)         # everything through the list kernels
        left_slow = eng.get_param("expand_stream_left_to_v1")
    finally:
        eng.set_param("expand_job_tiles", before)
    assert left == expect_left, (left, expect_left)
    assert left_slow == _n_tiles(b), (left_slow, _n_tiles(b))
    total = r3["total"]
    assert len(r3["out"]) == total + 64
    empty = b["op_off"][1:] == b["op_off"][:-1]
    for f in ("bad_op_idx", "panic_op_idx", "bad_base_pos"):
        assert (r3["diag"][f] == r0["diag"][f]).all(), f
        assert (rs["diag"][f] == r0["diag"][f]).all(), f
        assert (r3["diag"][f][empty] == NONE).all(), f
    c = r3["counts"]
    t_len, q_len = b["t_src_len"] + c["ins_bp"] + c["inv_ins_bp"], b["q_src_len"] + c["del_bp"] + c["inv_del_bp"]
    # a record the reference rejects has no rows to get right: v1's own two paths differ in what they leave at an invalid base
    # (its row emitters against its op-serial walk), so the run through the op-serial walk is compared outside such rows
    failed = np.zeros(total + 64, dtype=bool)
    for i in np.flatnonzero((r0["diag"]["bad_op_idx"] != NONE) | (r0["diag"]["panic_op_idx"] != NONE) |
                            (r0["diag"]["bad_base_pos"] != NONE)):
        failed[int(r3["t_row_off"][i]):int(r3["t_row_off"][i]) + int(t_len[i])] = True
        failed[int(r3["q_row_off"][i]):int(r3["q_row_off"][i]) + int(q_len[i])] = True
    for name, r, where in (("stream", r3, slice(None)), ("force_slow", rs, ~failed)):
        if not (r["out"][where] == r0["out"][where]).all():
            k = int(np.flatnonzero((r["out"] != r0["out"]) & (True if name == "stream" else ~failed))[0])
            raise AssertionError("%s: byte %d differs from v1: %#x vs %#x" % (name, k, int(r["out"][k]), int(r0["out"][k])))
    # bytes outside the rows the layout gives, and the canary behind them
    covered = np.zeros(total + 64, dtype=bool)
    for off, ln in ((r3["t_row_off"], t_len), (r3["q_row_off"], q_len)):
        for o, l in zip(off.tolist(), ln.tolist()):
            covered[int(o):int(o) + int(l)] = True
    assert not covered[total:].any()
    assert (r3["out"][~covered] == FILL).all(), np.flatnonzero(r3["out"][~covered] != FILL)[:5]


EXPECT_LEFT = {"lengths": lambda jt: 0, "edges": lambda jt: 3, "job": lambda jt: jt, "jobs": lambda jt: 2 * jt}


def check_paf2maf(eng, jt):
    for name, b in all_batches(jt):
        check_paf2maf_batch(eng, b, jt, EXPECT_LEFT[name](jt))


def run_pafpseudo(eng, b, base_mode, skip, dst_off, out_bytes, variant):
    """wga_cigar_class_sums + wga_pafpseudo_fill into a pre-filled buffer; host copies of the buffer and the diagnostics"""
    before = eng.get_param("pseudo_variant")
    eng.set_param("pseudo_variant", variant)
    try:
        batch = eng.make_batch(b["ops"], b["op_off"], b["strand_neg"])
        eng.cigar_class_sums(batch)
        out = eng.empty(out_bytes, np.uint8).fill(FILL)
        if base_mode:
            diag = eng.pafpseudo_fill(batch, 1, eng.upload(b["q_pool"]), len(b["q_pool"]), eng.upload(b["q_src_off"]),
                                      eng.upload(b["q_src_len"]), eng.upload(skip), out, eng.upload(dst_off))
        else:
            diag = eng.pafpseudo_fill(batch, 0, None, 0, None, None, eng.upload(skip), out, eng.upload(dst_off))
        return out.numpy(), diag.numpy(), eng.get_param("pseudo_stream_left_to_blocks") if variant == 3 else 0
    finally:
        eng.set_param("pseudo_variant", before)


def check_pafpseudo_batch(eng, b, base_mode, expect_left):
    """pafpseudo's streaming kernel == its block kernel over the whole buffer and the diagnostics; the records with ops against
    the oracle; fill outside the segments.  A record's head is trimmed by a few columns now and then (the switch sets the first
    written column)."""
    n = len(b["strand_neg"])
    sums = pc.expected_class_sums(b["ops"], b["op_off"])
    cols = (sums["mx"] + sums["d"]).astype(np.int64)
    skip = np.minimum(cols, (np.arange(n) % 4) * 3).astype(np.uint64)
    if base_mode:
        seg = b["q_src_len"].astype(np.int64) - (sums["i"] + sums["s"]).astype(np.int64) + sums["d"].astype(np.int64)
    else:
        seg = cols.copy()
    seg = np.maximum(seg - skip.astype(np.int64), 0)
    gaps = np.random.default_rng(n).integers(0, 20, n)
    dst_off = np.zeros(n, dtype=np.uint64)
    dst_off[1:] = np.cumsum(seg + gaps)[:-1]
    dst_off += np.uint64(3)
    out_bytes = 3 + int((seg + gaps).sum()) + 64
    o3, d3, left = run_pafpseudo(eng, b, base_mode, skip, dst_off, out_bytes, 3)
    o0, d0, _ = run_pafpseudo(eng, b, base_mode, skip, dst_off, out_bytes, 0)
    assert left == expect_left, (left, expect_left)
    for f in ("panic_op_idx", "bad_base_pos"):
        assert (d3[f] == d0[f]).all(), f
    if not (o3 == o0).all():
        k = int(np.flatnonzero(o3 != o0)[0])
        raise AssertionError("byte %d differs from the block kernel: %#x vs %#x" % (k, int(o3[k]), int(o0[k])))
    covered = np.zeros(out_bytes, dtype=bool)
    for i in range(n):
        covered[int(dst_off[i]):int(dst_off[i]) + int(seg[i])] = True
    assert (o3[~covered] == FILL).all(), np.flatnonzero(o3[~covered] != FILL)[:5]
    for i in _with_ops(b):
        q = b"" if not base_mode else b["q_pool"][int(b["q_src_off"][i]):int(b["q_src_off"][i] + b["q_src_len"][i])].tobytes()
        try:
            if base_mode and b["strand_neg"][i]:
                q = orc.reverse_complement(q)
            row = orc.gen_pesudo_maf_by_cigar(pc.text_any(pc.rec_ops(b, i)), q, bool(base_mode))[int(skip[i]):]
        except orc.OracleError as e:
            if e.kind == 4:
                assert int(d3["bad_base_pos"][i]) != NONE, i
            else:
                assert e.kind == 6 and int(d3["panic_op_idx"][i]) != NONE, (i, e.message)
            continue
        assert int(d3["panic_op_idx"][i]) == NONE and int(d3["bad_base_pos"][i]) == NONE, (i, d3[i])
        assert len(row) == int(seg[i]), (i, len(row), seg[i])
        assert o3[int(dst_off[i]):int(dst_off[i]) + len(row)].tobytes() == row, i


def check_pafpseudo(eng, jt):
    """the same layouts through pafpseudo's two modes (they share the stream)"""
    before = eng.get_param("expand_job_tiles")
    eng.set_param("expand_job_tiles", jt)
    try:
        for name, b in all_batches(jt):
            check_pafpseudo_batch(eng, b, 0, 0)     # symbol mode: no slices, nothing is left to the block kernel
            check_pafpseudo_batch(eng, b, 1, EXPECT_LEFT[name](jt))
    finally:
        eng.set_param("expand_job_tiles", before)
