"""`maf2paf` on the device (K28): the C-ABI entry (Engine.maf2paf) against maf2paf_ref.maf2paf_ref, the restatement that works
from the arrays, against K11's cg:Z: text for the same runs, and the `wgatools maf2paf` command with its device writer against
its host writer.
Imported by test_emu_maf2paf.py (emulator build, CPU) and test_gpu_maf2paf.py (the product on a GPU); each provides the `cli`
and `eng` fixtures."""
import ctypes as C
import os
import random
import re
import subprocess

import numpy as np

import maf2paf_ref as ref
import text_items_cases as ti
from chain2paf_cases import QUOTED
from chain_split_cases import run, write
from wgatools_amd.engine import COUNTS_DTYPE, MAF2PAF_HEAD_DTYPE, MAF_LINE_DTYPE

U64 = (1 << 64) - 1
E_INVALID_ARG = -1
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SIX = ("match", "mismatch", "ins_bp", "inv_ins_bp", "del_bp", "inv_del_bp")
ITEM = re.compile(rb"[0-9]+[=IDX]")      # a run's part of the cg:Z: text


# ---- arrays ----------------------------------------------------------------------------------------------------------------------
def rec(n_runs, k=0, qname=b"qchr", tname=b"tchr", q=(90000, 7, 57), t=(100000, 10, 60), neg=False, runs=None, cols=None,
        counts=None):
    """a block: n_runs runs of 1 + (j + k) % 7 columns in the classes = I D X in turn, or `runs` as (start, class) pairs with
    `cols`; counts: the six terms of block_length in SIX's order (else the runs' columns by class)"""
    if runs is None:
        runs, at = [], 0
        for j in range(n_runs):
            runs.append((at, (j + k) % 4))
            at += 1 + (j + k) % 7
        cols = at
    if counts is None:
        by = [0, 0, 0, 0]
        for j, (start, cls) in enumerate(runs):
            end = runs[j + 1][0] if j + 1 < len(runs) else cols
            by[min(cls, 3)] += (end - start) & U64
        counts = (by[0], by[3], by[1], 0, by[2], 0) if not neg else (by[0], by[3], 0, by[1], 0, by[2])
    return dict(qname=qname, tname=tname, q=q, t=t, neg=neg, runs=runs, cols=cols, counts=counts)


class Arrays:
    """the arrays of wga_maf2paf for a list of blocks, on the device and on the host; the names back to back in one buffer"""

    def __init__(self, eng, recs, run_off=None):
        self.eng, self.n = eng, len(recs)
        names = bytearray()
        self.heads = np.zeros(self.n + 1, dtype=MAF2PAF_HEAD_DTYPE)
        self.counts = np.zeros(self.n + 1, dtype=COUNTS_DTYPE)
        runs, off, cols = [], [0], []
        for r, b in enumerate(recs):
            h = self.heads[r]
            h["q"], h["t"], h["strand_neg"] = b["q"], b["t"], 1 if b["neg"] else 0
            h["qname_off"], h["qname_len"] = len(names), len(b["qname"])
            names += b["qname"]
            h["tname_off"], h["tname_len"] = len(names), len(b["tname"])
            names += b["tname"]
            for key, v in zip(SIX, b["counts"]):
                self.counts[r][key] = v
            self.counts[r]["ins_ev"], self.counts[r]["inv_ev"] = 0x1111111111111111, U64       # not terms of the sums
            runs += [(start << 3 | cls) & U64 for start, cls in b["runs"]]
            off.append(len(runs))
            cols.append(b["cols"] & U64)
        self.names = bytes(names)
        self.runs = np.array(runs + [0], dtype=np.uint64)
        self.off = np.array(off if run_off is None else run_off, dtype=np.uint64)
        self.cols = np.array(cols + [0], dtype=np.uint64)
        self.nr = len(runs)
        self.upload()

    def upload(self):
        eng = self.eng
        self.d_names = eng.upload(np.frombuffer(self.names + b"\0" * 16, dtype=np.uint8))
        self.d_heads, self.d_counts = eng.upload(self.heads), eng.upload(self.counts)
        self.d_runs, self.d_off, self.d_cols = eng.upload(self.runs), eng.upload(self.off), eng.upload(self.cols)

    def args(self):
        return self.n, self.d_names, len(self.names), self.d_heads, self.d_counts, self.d_runs, self.d_off, self.d_cols

    def want(self):
        return ref.maf2paf_ref(self.heads[:self.n], self.counts, self.runs, self.off, self.cols, self.names)


def check(eng, recs, a=None, shift=0):
    """the device's bytes and its count are the restatement's; the guards around d_out are checked inside Engine.maf2paf"""
    a = a or Arrays(eng, recs)
    text = eng.maf2paf(*a.args(), out_shift=shift)
    exp = a.want()
    assert text == exp, (shift, len(text), len(exp), text[:300], exp[:300])
    return text


# ---- ABI level -----------------------------------------------------------------------------------------------------------------
def check_abi_fill_block_edges(eng):
    """256 items per block of the fill: one block of n runs is n + 1 items; with a second block behind it that block's head is
    item n + 1"""
    for n in (254, 255, 256, 257, 513):
        text = check(eng, [rec(n)])
        assert text.count(b"\n") == 1 and len(ITEM.findall(text.split(b"cg:Z:")[1])) == n
        text = check(eng, [rec(n), rec(3, 1, tname=b"second")])
        assert text.count(b"\n") == 2 and text.endswith(b"\tsecond\t100000\t10\t60\t0\t9\t255\tNM:i:9\tcg:Z:2I3D4X\n")


def check_abi_plan_edges(eng):
    """256 blocks per block of the plan pass"""
    for n in (255, 256, 257, 700):
        text = check(eng, [rec(1, 0, t=(100000, 0, k % 5)) for k in range(n)])
        assert text.count(b"\t1\t1\t255\tNM:i:0\tcg:Z:1=\n") == n


def wide_runs(n):
    """n runs whose lengths are as wide as a u64 prints.  Starts are u64 >> 3, below 2^61, so ascending starts 10^18 apart end
    after two runs; these alternate between 0 and 2^60 instead: the lengths are 2^60 (19 digits, an item of 20 bytes) and 2^64 -
    2^60 (the difference wraps: 20 digits, 21 bytes)"""
    return [((j % 2) << 60, j % 8) for j in range(n)]


def widest_runs(n):
    """n runs of descending starts: every length wraps to 2^64 - 1, 20 digits: items of 21 bytes, 22 with the record's end — the
    widest a run item can be"""
    return [((1 << 60) - j, j % 8) for j in range(n)]


def check_abi_stage_limit(eng):
    """600 runs of maximal width, alone and between short blocks: the widest blocks of items the stage takes"""
    for runs, cols, sizes in ((wide_runs(600), 1 << 61, {20, 21}), (widest_runs(600), (1 << 60) - 600, {21})):
        big = rec(0, runs=runs, cols=cols, counts=(0,) * 6)
        cg = check(eng, [big]).split(b"cg:Z:")[1]
        items = ITEM.findall(cg)
        assert len(items) == 600 and set(len(i) for i in items) == sizes and len(cg) == sum(len(i) for i in items) + 1
        check(eng, [rec(2), big, rec(2, 1)])
    assert len(cg) == 600 * 21 + 1 and cg.startswith(b"%d=%dI" % (U64, U64))


def check_abi_over_the_stage(eng):
    """heads with names of 3 000 bytes (staged: the block's stretch stays below the stage of 6 144 bytes) and 20 000 bytes
    (direct): as target, as query, and both, among short blocks"""
    for n in (3000, 20000):
        for recs in ([rec(3), rec(4, 1, tname=b"T" * n), rec(2, 2)], [rec(3), rec(5, 3, qname=b"Q" * n), rec(1, 4)],
                     [rec(2, 0, tname=b"t" * n, qname=b"q" * n)],
                     [rec(3), rec(4, 1, tname=b"T" * n), rec(2, 2), rec(5, 3, qname=b"Q" * n), rec(1, 4)],
                     [rec(300), rec(300, 1, tname=b"A" * n), rec(300, 2, qname=b"B" * n)]):
            assert len(check(eng, recs)) > n


def check_abi_values(eng):
    for v in (0, U64):                                                   # every head number
        want = b"qchr\t%d\t%d\t%d\t+\ttchr\t%d\t%d\t%d\t5\t5\t255\tNM:i:0\tcg:Z:5=\n" % ((v,) * 6)
        assert check(eng, [rec(0, q=(v,) * 3, t=(v,) * 3, runs=[(0, 0)], cols=5)]) == want
    # the six terms wrap 2^64: (2^64 - 10) + 3 + 4 + 5 + 6 + 7 = 15, NM = 15 - (2^64 - 10) = 25
    text = check(eng, [rec(2), rec(1, counts=(U64 - 9, 3, 4, 5, 6, 7)), rec(2, 1)])
    assert text.split(b"\n")[1].split(b"\t")[9:13] == [b"%d" % (U64 - 9), b"15", b"255", b"NM:i:25"]
    text = check(eng, [rec(1, counts=(1 << 63, 1 << 63, 1 << 63, 1 << 63, 7, 0))])
    assert text.split(b"\t")[9:13] == [b"%d" % (1 << 63), b"7", b"255", b"NM:i:%d" % ((7 - (1 << 63)) & U64)]
    assert check(eng, [rec(1, counts=(0, 0, 0, 0, 0, 0))]).split(b"\t")[9:13] == [b"0", b"0", b"255", b"NM:i:0"]
    assert check(eng, [rec(1, counts=(U64,) * 6)]).split(b"\t")[9:13] == [b"%d" % U64, b"%d" % (U64 - 5), b"255", b"NM:i:%d" % (U64 - 4)]
    for neg in (False, True):                                            # both strands
        f = check(eng, [rec(4, neg=neg)]).split(b"\t")
        assert f[4] == (b"-" if neg else b"+") and len(f) == 14
    assert check(eng, [rec(0)]) == b"qchr\t90000\t7\t57\t+\ttchr\t100000\t10\t60\t0\t0\t255\tNM:i:0\tcg:Z:\n"     # no runs
    assert check(eng, [rec(2), rec(0, 1), rec(3, 2)]).count(b"\tcg:Z:\n") == 1
    classes = rec(0, runs=[(3 * c, c) for c in range(8)], cols=30, counts=(3, 0, 3, 0, 3, 15 + 6))
    assert check(eng, [classes]).endswith(b"\t3\t30\t255\tNM:i:27\tcg:Z:3=3I3D3X3X3X3X9X\n")


SPECIAL = (b"a\tb", b"\t", b"c\rd", b"e\nf", b"\r\n", b'g"\th\n')


def check_abi_quoting(eng):
    """a name with a quote, a tab, CR or LF goes between quotes, the quotes inside doubled: as query, as target, and both; the
    count is the restatement's length (Engine.maf2paf allocates by it and checks the guards)"""
    plain, front = check(eng, [rec(2)]), len(check(eng, [rec(3)]))
    for name in QUOTED + SPECIAL:
        q = b'"' + name.replace(b'"', b'""') + b'"'
        as_q = check(eng, [rec(3), rec(2, 0, qname=name), rec(1, 1)])
        assert as_q[front:].startswith(plain.replace(b"qchr", q))
        as_t = check(eng, [rec(2, 0, tname=name), rec(300, 1)])
        assert as_t.startswith(plain.replace(b"tchr", q))
        assert check(eng, [rec(2, 0, tname=name, qname=name)]) == plain.replace(b"qchr", q).replace(b"tchr", q)
    names = QUOTED[:4] + SPECIAL
    check(eng, [rec(1 + k % 3, k, tname=names[k % len(names)], qname=names[(k + 1) % len(names)]) for k in range(300)])


def random_arrays(eng, seed, n=300, max_runs=12):
    """arrays that no MAF gives: any class 0 .. 7, ascending starts of any size below 2^61, blocks without runs"""
    rnd = random.Random(seed)
    recs = []
    for k in range(n):
        runs, at = [], rnd.randrange(3)
        for _ in range(rnd.randrange(max_runs + 1)):
            runs.append((at, rnd.randrange(8)))
            at += rnd.choice((1, 1, 2, 9, 10, 99, 1234, 10 ** 6, 10 ** rnd.randrange(17)))
        recs.append(rec(0, runs=runs, cols=at, qname=b"q%d" % k, tname=b"t%d" % (k % 7), neg=rnd.random() < 0.5,
                        q=tuple(rnd.randrange(1 << rnd.randrange(1, 65)) for _ in range(3)),
                        t=tuple(rnd.randrange(1 << rnd.randrange(1, 65)) for _ in range(3))))
    return Arrays(eng, recs)


def check_abi_cross_k11(eng):
    """the bytes behind `cg:Z:` of every record are wga_maf_runs_cigar_text's for the same runs, run_off and cols"""
    for seed in (0, 1, 2):
        a = random_arrays(eng, seed)
        cnt = eng.maf_runs_cigar_text(a.n, a.nr, a.d_runs, a.d_off, a.d_cols)
        off = eng.exclusive_scan_u64(a.n, cnt)
        o = [int(v) for v in off.numpy()]
        out = eng.empty(o[-1] + 64, np.uint8).fill(0)
        eng.maf_runs_cigar_text(a.n, a.nr, a.d_runs, a.d_off, a.d_cols, out=out, out_off=off)
        eng.sync()
        k11 = out.numpy().tobytes()
        lines = check(eng, None, a=a).split(b"\n")
        assert len(lines) == a.n + 1 and lines[-1] == b""
        for r in range(a.n):
            assert lines[r].split(b"\tcg:Z:")[1] == k11[o[r]:o[r + 1]], (seed, r)


def check_abi_hand_built(eng):
    """run_off with equal neighbours (blocks without runs first, in the middle, last, and only heads across the fill's blocks),
    name spans that do not lie inside d_names, n == 0"""
    recs = [rec(2, 0), rec(3, 1), rec(1, 2), rec(2, 3)]
    assert Arrays(eng, recs).off.tolist() == [0, 2, 5, 6, 8]
    for off, empties in (([0, 0, 5, 5, 8], 2), ([0, 3, 3, 8, 8], 2), ([0, 0, 0, 0, 8], 3), ([0, 8, 8, 8, 8], 3)):
        a = Arrays(eng, recs, run_off=off)
        text = check(eng, None, a=a)
        assert text.count(b"\n") == 4 and text.count(b"\tcg:Z:\n") == empties, off
    many = [rec(1, k) for k in range(600)]
    assert check(eng, None, a=Arrays(eng, many, run_off=[0] * 300 + list(range(0, 301)))).count(b"\n") == 600
    # spans outside the names: behind the end, across the end, an offset of 2^64 - 1; a span that ends at the end is inside
    a = Arrays(eng, recs)
    nb = len(a.names)
    a.heads[0]["qname_off"], a.heads[0]["qname_len"] = nb, 1
    a.heads[1]["tname_off"], a.heads[1]["tname_len"] = nb - 2, 3
    a.heads[2]["qname_off"], a.heads[2]["qname_len"] = U64, 4
    a.heads[2]["tname_off"], a.heads[2]["tname_len"] = 1 << 40, 0xFFFFFFFF
    a.heads[3]["tname_off"], a.heads[3]["tname_len"] = nb - 3, 3
    a.upload()
    lines = check(eng, None, a=a).split(b"\n")
    assert lines[0].startswith(b"\t90000\t") and lines[1].split(b"\t")[5] == b"" and lines[2].split(b"\t")[0::5][:2] == [b"", b""]
    assert lines[3].split(b"\t")[5] == b"chr"
    none = eng.upload(np.zeros(1, dtype=np.uint64))
    assert eng.maf2paf(0, a.d_names, nb, a.d_heads, a.d_counts, a.d_runs, none, a.d_cols) == b""           # n == 0
    assert eng.maf2paf(0, None, 0, None, None, None, None, None) == b""
    assert check(eng, None, a=a) == b"\n".join(lines)                                                      # ... and again


def check_abi_alignment(eng):
    """records of one odd length, one after the other: they start at every offset within a 16-byte group; d_out at every offset
    behind an aligned address"""
    one = check(eng, [rec(1)])
    pad = b"n" * (1 + len(one) % 2)
    recs = [rec(1, 0, qname=b"qchr" + pad) for _ in range(20)] + [rec(1 + k % 3, k, tname=b"t" * (k + 1)) for k in range(9)]
    a = Arrays(eng, recs)
    text = check(eng, None, a=a)
    starts, at = set(), 0
    for line in text.split(b"\n")[:-1]:
        starts.add(at % 16)
        at += len(line) + 1
    assert starts == set(range(16)), starts
    small = Arrays(eng, [rec(3), rec(1, 1, tname=b'abc"defg'), rec(40, 2)])
    for shift in range(16):
        check(eng, None, a=small, shift=shift)
        check(eng, None, a=a, shift=shift)


def check_abi_count_fill(eng):
    """*total_bytes is the restatement's length, also from a workspace that other arrays' calls used before; the second call
    leaves it alone (Engine._count_then_fill raises when it does not)"""
    work = eng.empty(int(eng.lib.wga_maf2paf_work_bytes(130, 3000)), np.uint8)
    for seed in (0, 1):
        a = Arrays(eng, [rec(1 + (k + seed) % 40, k, qname=b"q%d" % k) for k in range(120 + seed)])
        want = a.want()
        assert eng.maf2paf_count(*a.args(), work) == len(want)
        assert eng.maf2paf(*a.args(), work=work) == want


def item_stream(eng):
    """one block of 300 runs and one of 298: 600 items, three blocks of the fill.  The scan of the item sizes stands behind the
    plan and the sums in d_work, at word 3 n (capi_maf2paf.inc)"""
    a = Arrays(eng, [rec(300), rec(298, 1, tname=b"second")])
    work = eng.empty(int(eng.lib.wga_maf2paf_work_bytes(a.n, a.nr)), np.uint8)
    want = a.want()
    assert eng.maf2paf_count(*a.args(), work) == len(want)

    def fill(total_bytes, d_out):
        tot = C.c_uint64(total_bytes)
        n, names, nb, heads, counts, runs, off, cols = a.args()
        assert eng.lib.wga_maf2paf(eng.ctx, n, names.ptr, nb, heads.ptr, counts.ptr, runs.ptr, off.ptr, cols.ptr, work.ptr,
                                   C.byref(tot), d_out) == 0
        assert tot.value == total_bytes
    return ti.Stream(eng, work, 3 * a.n, a.n + a.nr, want, fill)


def check_abi_fill_short_total(eng):
    ti.check_short_total(item_stream(eng))


def check_abi_fill_scan_one_off(eng):
    ti.check_scan_one_off(item_stream(eng), size_checked=False)


def raw(eng, a, n=None, d_off=None, work=True, null=()):
    d_work = eng.empty(max(int(eng.lib.wga_maf2paf_work_bytes(a.n, a.nr)), 16), np.uint8)
    total = C.c_uint64(7)
    p = dict(names=a.d_names.ptr, heads=a.d_heads.ptr, counts=a.d_counts.ptr, runs=a.d_runs.ptr,
             off=(a.d_off if d_off is None else d_off).ptr, cols=a.d_cols.ptr)
    for k in null:
        p[k] = None
    rc = eng.lib.wga_maf2paf(eng.ctx, a.n if n is None else n, p["names"], len(a.names), p["heads"], p["counts"], p["runs"], p["off"],
                             p["cols"], d_work.ptr if work else None, C.byref(total), None)
    return rc, total.value


def check_abi_arguments(eng):
    a = Arrays(eng, [rec(3), rec(2, 1)])
    assert raw(eng, a) == (0, len(a.want()))
    assert raw(eng, a, work=False)[0] == E_INVALID_ARG
    assert raw(eng, a, work=False, n=0)[0] == E_INVALID_ARG                     # a null d_work, whatever the counts
    for null in ("names", "heads", "counts", "runs", "off", "cols"):
        assert raw(eng, a, null=(null,))[0] == E_INVALID_ARG, null
        assert raw(eng, a, n=0, null=(null,)) == (0, 0), null
    assert raw(eng, a, n=0) == (0, 0)                                           # n == 0: total 0
    # n + runs beyond 0xFFFFFFF0: the call reads the number of runs from the last offset and refuses (counts only)
    assert raw(eng, a, d_off=eng.upload(np.array([0, 3, 0xFFFFFFF0 - 1], dtype=np.uint64)))[0] == E_INVALID_ARG
    assert raw(eng, a, d_off=eng.upload(np.array([0, 3, U64], dtype=np.uint64)))[0] == E_INVALID_ARG
    assert int(eng.lib.wga_maf2paf_work_bytes(0, 0)) >= 8
    assert int(eng.lib.wga_maf2paf_work_bytes(1000, 30000)) == 8 * (3 * 1000 + 31000 + 1 + 31000 // 1024 + 4)


# ---- random MAF text through the splitter and K3 --------------------------------------------------------------------------------
def random_maf(seed, n_blocks=None, max_cols=300, names=None):
    """(text, blocks): blocks of two rows over ACGT and gaps (never a gap in both rows of a column), the query on either
    strand; blocks = (tname, t numbers, qname, q numbers, neg, t row, q row)"""
    rnd = random.Random(1000 + seed)
    n_blocks = n_blocks or 150 + (seed * 53) % 250
    out, blocks = [b"##maf version=1 scoring=none\n"], []
    for k in range(n_blocks):
        cols = rnd.randrange(1, max_cols + 1)
        trow, qrow = bytearray(), bytearray()
        mode, left = 0, 0
        for _ in range(cols):
            if left == 0:
                mode, left = rnd.choice((0, 0, 0, 1, 2, 3)), rnd.randrange(1, 12)
            left -= 1
            b = rnd.choice(b"ACGT")
            if mode == 0:
                trow.append(b), qrow.append(b)
            elif mode == 1:
                trow.append(ord("-")), qrow.append(b)
            elif mode == 2:
                trow.append(b), qrow.append(ord("-"))
            else:
                trow.append(b), qrow.append(rnd.choice(bytes(set(b"ACGT") - {b})))
        tn, qn = (names or (b"ref.chr%d" % (k % 5), b"qry.ctg%d" % (k % 11)))
        t = (rnd.randrange(10 ** 4), cols - trow.count(b"-"), 10 ** 6 + rnd.randrange(10 ** 9))
        q = (rnd.randrange(10 ** 4), cols - qrow.count(b"-"), 10 ** 6 + rnd.randrange(10 ** 9))
        neg = rnd.random() < 0.4
        sep = rnd.choice((b" ", b"\t", b"  "))
        out.append(b"a score=%d\n" % k)
        out.append(sep.join((b"s", tn, b"%d" % t[0], b"%d" % t[1], b"+", b"%d" % t[2], bytes(trow))) + b"\n")
        out.append(sep.join((b"s", qn, b"%d" % q[0], b"%d" % q[1], b"-" if neg else b"+", b"%d" % q[2], bytes(qrow))) + b"\n\n")
        blocks.append((tn, t, qn, q, neg, bytes(trow), bytes(qrow)))
    return b"".join(out), blocks


def expected_paf(blocks):
    """maf.rs:484-520 on the rows themselves: a column is I where the target has a gap, D where the query has one, = where the
    bases are equal, X otherwise"""
    out = []
    for tn, t, qn, q, neg, trow, qrow in blocks:
        cg, prev, n, matches = [], None, 0, 0
        for a, b in zip(trow, qrow):
            c = "I" if a == 45 else "D" if b == 45 else "=" if a == b else "X"
            matches += c == "="
            if c != prev and prev is not None:
                cg.append("%d%s" % (n, prev))
                n = 0
            prev, n = c, n + 1
        cg.append("%d%s" % (n, prev))
        qs, qe = (q[2] - q[0] - q[1], q[2] - q[0]) if neg else (q[0], q[0] + q[1])
        out.append(b"\t".join([qn] + [b"%d" % v for v in (q[2], qs, qe)] + [b"-" if neg else b"+", tn] +
                              [b"%d" % v for v in (t[2], t[0], t[0] + t[1], matches, len(trow), 255)] +
                              [b"NM:i:%d" % (len(trow) - matches), b"cg:Z:" + "".join(cg).encode()]) + b"\n")
    return b"".join(out)


def check_abi_random_files(eng, seeds=range(12)):
    """random MAF text -> Engine.maf_split -> wga_maf_pair_stat (both calls) -> wga_maf2paf with the names where the splitter
    found them in the uploaded file: the restatement's bytes from the arrays, and the expected records from the rows"""
    for seed in seeds:
        text, blocks = random_maf(seed)
        d_text = eng.upload(np.frombuffer(text + b"\0" * 16, dtype=np.uint8))
        nl = eng.maf_split(d_text, len(text))
        d_lines = eng.empty(nl + 1, MAF_LINE_DTYPE)
        assert eng.maf_split(d_text, len(text), d_lines) == nl
        s = [ln for ln in d_lines.numpy()[:nl] if int(ln["status"]) == 0]
        n = len(blocks)
        assert len(s) == 2 * n and 150 <= n < 400
        heads = np.zeros(n + 1, dtype=MAF2PAF_HEAD_DTYPE)
        t_off, q_off, cols, strand = [], [], [], []
        for r in range(n):
            t, q = s[2 * r], s[2 * r + 1]
            (ts, tl, tz), (qs, ql, qz) = [int(v) for v in t["num"]], [int(v) for v in q["num"]]
            neg = bool(q["strand_neg"])
            heads[r]["q"] = (qz, qz - qs - ql, qz - qs) if neg else (qz, qs, qs + ql)
            heads[r]["t"] = (tz, ts, ts + tl)
            heads[r]["strand_neg"] = neg
            heads[r]["qname_off"], heads[r]["qname_len"] = q["name_off"], q["name_len"]
            heads[r]["tname_off"], heads[r]["tname_len"] = t["name_off"], t["name_len"]
            t_off.append(int(t["seq_off"])), q_off.append(int(q["seq_off"]))
            cols.append(min(int(t["seq_len"]), int(q["seq_len"]))), strand.append(1 if neg else 0)
        d_t, d_q = eng.upload(np.array(t_off, dtype=np.uint64)), eng.upload(np.array(q_off, dtype=np.uint64))
        d_c, d_s = eng.upload(np.array(cols, dtype=np.uint64)), eng.upload(np.array(strand, dtype=np.uint8))
        counts, run_cnt = eng.maf_pair_stat(n, d_text, d_t, d_q, d_c, d_s)
        run_off = eng.exclusive_scan_u64(n, run_cnt)
        off = run_off.numpy()
        runs = eng.empty(int(off[-1]) + 1, np.uint64).fill(0)
        eng.maf_pair_stat(n, d_text, d_t, d_q, d_c, d_s, counts=counts, run_cnt=run_cnt, runs=runs, run_off=run_off)
        got = eng.maf2paf(n, d_text, len(text), eng.upload(heads), counts, runs, run_off, d_c)
        assert got == ref.maf2paf_ref(heads[:n], counts.numpy(), runs.numpy(), off, cols, text), seed
        assert got == expected_paf(blocks), seed


# ---- command level -----------------------------------------------------------------------------------------------------------------
HOST_WRITER = {"WGA_MAF2PAF_WRITER": "host"}
FIXTURE = (b"query.chr8\t183119688\t181989421\t181990428\t+\tref.chr8\t182411202\t181469925\t181470925\t990\t1008\t255\tNM:i:18\t"
           b"cg:Z:109=1D243=1X12=1X138=1X177=1X31=1X133=8I18=1X100=2X7=1X22=\n")       # cli_cases.py::test_maf2paf_fixture


def timed(cli, args, env):
    """the command under WGA_TIMING=1: (exit status, stdout, the message without the timing lines, the timing lines)"""
    r = subprocess.run([cli] + list(args), stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=dict(os.environ, WGA_TIMING="1", **env))
    err = r.stderr.decode(errors="replace").split("\n")
    msg = "\n".join(ln for ln in err if "[timing]" not in ln).strip()
    return r.returncode, r.stdout, re.split(r" (?:ERROR|WARN) ", msg, 1)[-1], "\n".join(ln for ln in err if "[timing]" in ln)


def both_writers(cli, *args, env=None):
    """the command under the device writer and under WGA_MAF2PAF_WRITER=host: the same bytes, exit status and message, and
    under WGA_TIMING=1 the phase named after the writer that ran"""
    env = env or {}
    dev, host = timed(cli, args, env), timed(cli, args, dict(env, **HOST_WRITER))
    assert dev[0] in (0, 1) and dev[:3] == host[:3], (args, dev[0], host[0], dev[2], host[2])
    if dev[0] == 0:
        assert "maf2paf records (device)" in dev[3] and "maf2paf records (host)" not in dev[3], dev[3]
        assert "maf2paf records (host)" in host[3] and "maf2paf records (device)" not in host[3], host[3]
    return dev[:3]


def check_cli_fixture(cli):
    assert both_writers(cli, "maf2paf", os.path.join(GOLDEN, "test.maf")) == (0, FIXTURE, "")


def check_cli_random(cli, tmp_path):
    text, blocks = random_maf(3, n_blocks=120)
    assert both_writers(cli, "maf2paf", write(tmp_path, "r.maf", text)) == (0, expected_paf(blocks), "")


def check_cli_quoted(cli, tmp_path):
    """a name with a quote: the splitter takes the file, the device writer quotes the name"""
    text, blocks = random_maf(4, n_blocks=40, names=(b'ref"chr', b'"q"'))
    got = both_writers(cli, "maf2paf", write(tmp_path, "q.maf", text))
    assert got[0] == 0 and got[1].count(b'"""q"""\t') == 40 and got[1].count(b'\t"ref""chr"\t') == 40
    assert got[1] == expected_paf([(ref.csv_field(b[0]), b[1], ref.csv_field(b[2])) + b[3:] for b in blocks])


def check_cli_host_reader(cli, tmp_path):
    """files the host reader takes: CR line ends, and a name that is not ASCII; the names are gathered and uploaded"""
    text, blocks = random_maf(5, n_blocks=60)
    want = expected_paf(blocks)
    assert both_writers(cli, "maf2paf", write(tmp_path, "cr.maf", text.replace(b"\n", b"\r\n"))) == (0, want, "")
    assert both_writers(cli, "maf2paf", write(tmp_path, "h.maf", text), env={"WGA_MAF_READER": "host"}) == (0, want, "")
    name = "réf.chr".encode()
    text, blocks = random_maf(6, n_blocks=60, names=(name, b"qry"))
    got = both_writers(cli, "maf2paf", write(tmp_path, "u.maf", text))
    assert got == (0, expected_paf(blocks), "") and got[1].count(b"\t" + name + b"\t") == 60


def check_cli_query_name(cli, tmp_path):
    """-q <name> picks the query row by name: blocks of three rows, the third one (without gaps) named"""
    text, blocks = random_maf(7, n_blocks=50, names=(b"ref", b"mid"))
    three, blocks3 = [], []
    for k, part in enumerate(text.split(b"\n\n")[:-1]):
        tn, t, qn, q, neg, trow, qrow = blocks[k]
        row3 = bytes(b"ACGT"[(i * 7 + k) % 4] for i in range(len(trow)))
        three.append(part + b"\ns third %d %d + %d %s\n\n" % (k + 1, len(row3), 10 ** 6 + k, row3))
        blocks3.append((tn, t, b"third", (k + 1, len(row3), 10 ** 6 + k), False, trow, row3))
    path = write(tmp_path, "three.maf", b"".join(three))
    assert both_writers(cli, "maf2paf", path) == (0, expected_paf(blocks), "")
    assert both_writers(cli, "maf2paf", path, "-q", "third") == (0, expected_paf(blocks3), "")
    assert both_writers(cli, "maf2paf", path, "-q", "nobody")[0] == 1


def check_cli_pieces(cli, tmp_path):
    """several pieces (WGA_CHUNK_BYTES): every piece goes through the writer, the pieces' texts meet in order"""
    text, blocks = random_maf(8, n_blocks=60)
    path = write(tmp_path, "p.maf", text)
    one = both_writers(cli, "maf2paf", path)
    assert one == (0, expected_paf(blocks), "")
    for chunk in ("3000", "9000"):
        assert both_writers(cli, "maf2paf", path, env={"WGA_CHUNK_BYTES": chunk}) == one, chunk


def check_cli_gpus(cli, tmp_path, gpus=2):
    """--gpus N: the other devices' ranges get their names gathered and uploaded; the bytes of one device"""
    text, blocks = random_maf(9, n_blocks=80)
    path = write(tmp_path, "g.maf", text)
    one = both_writers(cli, "maf2paf", path)
    assert one == (0, expected_paf(blocks), "")
    assert both_writers(cli, "--gpus", str(gpus), "maf2paf", path) == one
    text, blocks = random_maf(10, n_blocks=30, names=(b'ref"chr', b'"q"'))
    path = write(tmp_path, "gq.maf", text)
    assert both_writers(cli, "--gpus", str(gpus), "maf2paf", path) == both_writers(cli, "maf2paf", path)
