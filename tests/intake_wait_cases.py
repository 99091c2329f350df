"""Where the streaming row kernel (expand_variant 3 / pseudo_variant 3) hands ops and windows from one step to the next, written
once and run twice: tests/test_emu_intake_wait.py on the SIMT emulator, tests/test_gpu_intake_wait.py on an MI355X.

The kernel requests the next 256 ops in the first super-step behind an intake (or, where no super-step runs between two
intakes, behind the write loop), parks them in LDS and takes them in from there; a record switch reads the ops taken in last
back from LDS; a super-step requests the queued granules' windows and the plain windows and puts the queued ones together.
These batches put the op stream where each of those hand-overs decides the bytes:
  * intakes with no super-step between them: two, three and five intakes in a row of one-column ops (= / X, = / I, I only,
    = / D), each stretch starting on an intake border, with wide ops around them;
  * several super-steps per intake: 256 and more ops of 60 - 300 columns each, all four kinds;
  * record switches read back from the parked ops: records that end at op 1, 2, 3, 4, 5, 255 and 256 of an intake directly
    behind a record that ended in the same intake (two and three switches in one group of 256, one-op records, the deciding
    op in lane 0 and in lane 63), in front of one-column ops (no super-step) and of wide ops;
  * stream start and restart: a tile left to v1 directly in front of such intakes, the job's first intake, and a last intake
    that is partial (the op count is no multiple of 256: the request behind it lies beyond the job's end);
  * the merge round: long = runs (no queued granule), a gap every 64 columns (exactly 64 queued granules in four kilobytes),
    every 60, 32 and 16 (the more-than-64 rule ends the super-step early), rows of dashes only (I and D runs of thousands),
    short records at odd row offsets (partial first and last kilobytes with queued granules), and an invalid base in a '-'
    record far from any gap (a plain granule) and next to one (a queued granule).
Batches are three to five jobs long plus a partial tile.  Every comparison is equality of bytes / integers, made by
stream_switch_cases' checks: variant 3 against variant 0 over the whole pre-filled output buffer and the diagnostics, the rows
against the oracle (parity_cases.check_paf2maf), bytes outside the rows and the canary keep the fill; the same batches through
pafpseudo's two modes."""
import numpy as np

import stream_switch_cases as sc

TILE = sc.TILE
JOB_TILES = (1, 2, 8)
EQ, X, I, D = sc.EQ, sc.X, sc.I, sc.D
KINDS = ("quiet", "wide", "switch", "restart", "merge")


def _op(code, ln):
    return (int(ln) << 4) | int(code)


class _Builder:
    """records as explicit op lists.  kind 'long': a query slice one byte longer than the CIGAR consumes (its tiles are v1's);
    bad: indices (query bases consumed in front, in the record's own direction) of invalid bases; such a record is '-'"""

    def __init__(self, seed):
        self.rng = np.random.default_rng(seed)
        self.recs, self.kind, self.strand, self.bad = [], [], [], []
        self.p = 0

    def rec(self, ops, kind=0, strand=None, bad=()):
        ops = np.asarray(ops, dtype=np.uint32)
        assert len(ops) > 0
        self.recs.append(ops)
        self.kind.append(kind)
        self.strand.append(int(self.rng.integers(0, 2)) if strand is None else strand)
        self.bad.append(tuple(bad))
        if bad:
            self.strand[-1] = 1
        self.p += len(ops)

    # ---- op lists ----
    def small(self, n):
        """= runs of 1 - 9 with an edit of 1 - 3 between them, = at both ends"""
        rng = self.rng
        code = np.where(np.arange(n) % 2 == 0, EQ, rng.choice(np.array([X, I, D]), n, p=[0.4, 0.3, 0.3]))
        code[-1] = EQ
        ln = np.where(code == EQ, rng.integers(1, 10, n), rng.integers(1, 4, n))
        return [_op(c, l) for c, l in zip(code.tolist(), ln.tolist())]

    def wide(self, n):
        """ops of 60 - 300 columns, all four kinds, = at both ends"""
        rng = self.rng
        code = rng.choice(np.array([EQ, X, I, D]), n, p=[0.4, 0.2, 0.2, 0.2])
        code[0] = code[-1] = EQ
        return [_op(c, l) for c, l in zip(code.tolist(), rng.integers(60, 301, n).tolist())]

    def ones(self, n, codes):
        """one-column ops, the codes in turn"""
        return [_op(codes[k % len(codes)], 1) for k in range(n)]

    def period(self, n_pairs, run, gap_code, gap=1):
        return [_op(EQ, run), _op(gap_code, gap)] * n_pairs + [_op(EQ, run)]

    # ---- layout ----
    def to(self, target, ops_of=None, **kw):
        """one record of small ops (or ops_of(n)) that ends exactly at op `target`"""
        assert target > self.p, (target, self.p)
        self.rec((ops_of or self.small)(target - self.p), **kw)

    def align(self, m=256):
        """the next record starts on a multiple of m ops"""
        if self.p % m:
            self.to((self.p // m + 1) * m)

    def build(self):
        rng = self.rng
        n = len(self.recs)
        op_off = np.zeros(n + 1, dtype=np.uint64)
        op_off[1:] = np.cumsum([len(r) for r in self.recs])
        t_len, q_len = np.zeros(n, dtype=np.uint64), np.zeros(n, dtype=np.uint64)
        for i, o in enumerate(self.recs):
            code, ln = o & 15, (o >> 4).astype(np.int64)
            t_len[i] = int(ln[(code == EQ) | (code == X) | (code == D)].sum())
            q_len[i] = int(ln[(code == EQ) | (code == X) | (code == I)].sum())
        clean_q = q_len.copy()
        for i, k in enumerate(self.kind):
            if k == "long":
                q_len[i] += 1
        q_off = np.zeros(n, dtype=np.uint64)
        q_off[1:] = np.cumsum(q_len)[:-1]
        q_off += np.uint64(64)
        t_off = np.zeros(n, dtype=np.uint64)
        t_off[1:] = np.cumsum(t_len)[:-1]
        t_off += np.uint64(64)
        lut = np.frombuffer(b"ACGTacgtNn", dtype=np.uint8)
        t_pool = lut[rng.integers(0, len(lut), 64 + int(t_len.sum()) + 64)]
        q_pool = lut[rng.integers(0, len(lut), 64 + int(q_len.sum()) + 64)]
        for i in range(n):
            for idx in self.bad[i]:
                assert idx < int(clean_q[i])
                q_pool[int(q_off[i]) + int(q_len[i]) - 1 - idx] = ord("R")
        return dict(ops=np.concatenate(self.recs).astype(np.uint32), op_off=op_off,
                    strand_neg=np.asarray(self.strand, dtype=np.uint8), t_pool=t_pool, q_pool=q_pool, t_src_off=t_off,
                    q_src_off=q_off, t_src_len=t_len, q_src_len=q_len), self.left()

    def left(self):
        """tiles with an op of a record that is not clean: v1's"""
        tiles, p = set(), 0
        for o, k in zip(self.recs, self.kind):
            if k:
                tiles.update(range(p // TILE, (p + len(o) - 1) // TILE + 1))
            p += len(o)
        return len(tiles)


def _finish(b, jt, tail):
    """small ops up to the end of the third job (or of the job the batch has reached), then a partial tile of `tail` ops"""
    job = jt * TILE
    end = max(3 * job, (b.p // job + 1) * job)
    assert end <= 5 * job, (b.p, job)
    if end - b.p > 600:
        b.to(end - 300)
    b.to(end + tail)
    return b.build()


def quiet_batch(jt):
    """two, three and five intakes in a row without a super-step: in one record, and with two record switches in every intake"""
    b = _Builder(1100 + jt)
    b.rec(b.wide(256))                                  # the job's first intake is followed by several super-steps
    b.align()
    # a stretch of one-column ops is n intakes of at most 256 columns each; wide ops behind it in the same record
    b.rec(b.ones(2 * 256 - 1, (EQ, X)) + [_op(EQ, 1)] + b.wide(40))
    b.align()
    for k in range(3):                                  # three intakes, switches at ops 100 and 255 of each
        b.rec(b.ones(99, (EQ, D)) + [_op(EQ, 1)])
        b.rec(b.ones(154, (EQ, I)) + [_op(EQ, 1)])
        b.rec([_op(EQ, 1)])
    b.rec(b.wide(40))
    b.align()
    b.rec([_op(EQ, 1)] + b.ones(5 * 256 - 2, (I,)) + [_op(EQ, 1)] + b.wide(40))    # five: the target row is dashes, the FIFO fills
    return _finish(b, jt, 77)


def wide_batch(jt):
    """several super-steps per intake: every op is 60 - 300 columns"""
    b = _Builder(1200 + jt)
    b.rec(b.wide(700))
    b.rec(b.wide(256), strand=1)
    b.rec(b.wide(300), strand=0)
    b.align()
    b.rec(b.wide(256), strand=1)                        # exactly one intake
    return _finish(b, jt, 300)


def switch_batch(jt):
    """records that end at op 1, 2, 3, 4, 5, 255 and 256 of an intake behind a record that ended in the same intake"""
    b = _Builder(1300 + jt)
    b.rec(b.small(40))
    for behind, ends in (("ones", (1, 2, 3, 5, 255, 256)), ("wide", (4, 5, 255)), ("ones", (2, 4, 252, 253, 254, 255, 256)),
                         ("small", (1, 255)), ("wide", (1, 2, 3, 5, 255, 256))):
        b.align()
        base = b.p
        for e in ends:
            b.to(base + e)                              # one-op records where two ends are neighbours
        if behind == "ones":                            # no super-step behind the intake
            b.rec(b.ones(299, (EQ, X)) + [_op(EQ, 1)])
        elif behind == "wide":
            b.rec(b.wide(20))
        else:
            b.rec(b.small(50))
    return _finish(b, jt, 129)


def restart_batch(jt):
    """tiles left to v1 directly in front of the intakes above; the first and the last, partial intake of a job"""
    job = jt * TILE
    b = _Builder(1400 + jt)
    b.rec(b.ones(255, (EQ, X)) + [_op(EQ, 1)] + b.ones(200, (EQ, I)) + [_op(EQ, 1)])   # the job's first intake: no super-step
    b.to(TILE - 3)
    b.rec(b.small(2) + [_op(EQ, 3)], kind="long")       # tile 0 ... ends at the tile border: tile 1 restarts the stream
    b.rec([_op(EQ, 1)])                                 # ... with a one-op record, a switch at op 1 of the first intake
    b.rec([_op(EQ, 2)])
    b.rec(b.ones(600, (EQ, D)) + [_op(EQ, 1)])
    b.to(job + TILE - 1)
    b.rec(b.small(3), kind="long")                      # two tiles are v1's (the record crosses the border)
    b.rec(b.wide(256))                                  # restart in the middle of an intake's worth of wide ops
    return _finish(b, jt, 131)                          # the last intake has 131 ops


def merge_batch(jt):
    """the merge round and the plain windows"""
    b = _Builder(1500 + jt)
    b.rec([_op(EQ, 20000)], strand=1)                   # no queued granule in any super-step
    b.rec([_op(EQ, 9), _op(I, 9000), _op(EQ, 5), _op(D, 9000), _op(EQ, 30)])     # rows of dashes only
    for s in (0, 1):
        b.rec(b.period(100, 63, I), strand=s)           # a gap every 64 columns of the target row: exactly 64 queued in 4 KB
        b.rec(b.period(100, 63, D), strand=s)           # ... of the query row
    b.rec(b.period(80, 59, I) + b.period(80, 59, D), strand=1)     # 68 and more: the super-step ends early
    b.rec(b.period(100, 31, D) + b.period(150, 15, I, 2), strand=0)
    b.rec(b.period(70, 64, I) + b.period(70, 62, D, 3), strand=1)
    for k in range(12):                                 # short records: partial first and last kilobytes with queued granules
        b.rec([_op(EQ, 5 + k), _op(I, 2), _op(EQ, 7), _op(D, 3), _op(EQ, 9 + 3 * k)])
    # an invalid base in a '-' record: in plain granules of the query row (it has no gap here) ...
    b.rec([_op(EQ, 3000), _op(I, 1), _op(EQ, 3000)], bad=(1500,))
    b.rec([_op(EQ, 3000), _op(I, 1), _op(EQ, 3000)], bad=(3003,))
    # ... and in queued ones: the last base in front of a gap, the first behind one
    b.rec([_op(EQ, 3000), _op(D, 1), _op(EQ, 3000)], bad=(2999,))
    b.rec([_op(EQ, 3000), _op(D, 5), _op(EQ, 3000)], bad=(3000,))
    b.rec(b.small(60))
    return _finish(b, jt, 19)


BATCHES = dict(quiet=quiet_batch, wide=wide_batch, switch=switch_batch, restart=restart_batch, merge=merge_batch)


def check_paf2maf(eng, jt, kind):
    b, left = BATCHES[kind](jt)
    sc.check_paf2maf_batch(eng, b, jt, left)


def check_pafpseudo(eng, jt, kind):
    """the same batch through pafpseudo's symbol and base modes (they share the stream)"""
    b, left = BATCHES[kind](jt)
    before = eng.get_param("expand_job_tiles")
    eng.set_param("expand_job_tiles", jt)
    try:
        sc.check_pafpseudo_batch(eng, b, 0, 0)
        sc.check_pafpseudo_batch(eng, b, 1, left)
    finally:
        eng.set_param("expand_job_tiles", before)
