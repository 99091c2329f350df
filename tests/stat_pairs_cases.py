"""The merged table of `stat` on the device (K36): the C-ABI entries (Engine.stat_pairs, Engine.stat_pair_rows) against
stat_pairs_ref (the restatement from stat.rs:167-223, numpy.float32 adds in record order), and the command with its device path
against WGA_STAT_WRITER=host and the restatement over the oracle's counters.
Imported by test_emu_stat_pairs.py (emulator build, CPU) and test_gpu_stat_pairs.py (the product on a GPU); each provides the
`cli` and `eng` fixtures."""
import ctypes as C
import gzip
import os
import random

import numpy as np

import maf2paf_cases as m2p
import oracle_py as orc
import stat_pairs_ref as ref
import stat_rows_cases as k33
import text_items_cases as ti
from chain_split_cases import run, write
from stat_rows_cases import COUNTS, HOST_WRITER, counts, first_difference, rec
from wgatools_amd.engine import COUNTS_DTYPE, STAT_PAIR_DTYPE, STAT_ROW_HEAD_DTYPE

U64 = (1 << 64) - 1
E_INVALID_ARG, E_TOO_SMALL = -1, -5
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
GUARD32 = 0xA5A5A5A5


def tup(r):
    return (r["rname"], r["ref_size"], r["ref_start"], r["qname"], r["query_size"], r["query_start"], r["c"])


def same_f32(got_bits, want):
    """the bit pattern is the restatement's f32; any NaN stands for any NaN (the sign of 0 / 0 is the divider's own)"""
    return (np.isnan(want) and np.isnan(ref.rows_ref.f32_of_bits(got_bits))) or int(got_bits) == ref.f32_bits(want)


def compare(pairs, por, want, wpor, what):
    assert len(pairs) == len(want), (what, len(pairs), len(want))
    assert [int(v) for v in por] == wpor, what
    for g, (p, w) in enumerate(zip(pairs, want)):
        for f in ("first_rec", "n_recs", "ref_start", "query_start"):
            assert int(p[f]) == w[f], (what, g, f, int(p[f]), w[f])
        for f in ref.COUNT_FIELDS:
            assert int(p["sum"][f]) == w["sum"][f], (what, g, f, int(p["sum"][f]), w["sum"][f])
        assert same_f32(p["inv_size_bits"], w["inv_size"]), (what, g, hex(int(p["inv_size_bits"])), w["inv_size"])
        assert int(p["pad"]) == 0, (what, g)


def check(eng, recs, inv_in=None, seen=None, what=None):
    """both calls (Engine.stat_pairs checks the guards around both outputs and that n_pairs stays): every field of every pair and
    every record's pair are the restatement's.  seen: the records as the device is to see them (names of spans that are refused)"""
    a = k33.Arrays(eng, recs)
    d_inv = eng.upload(np.asarray(inv_in, dtype=np.uint32)) if inv_in is not None else None
    pairs, por = eng.stat_pairs(*a.args(), inv_in=d_inv)
    want, wpor = ref.pairs([tup(r) for r in (seen or recs)], inv_in)
    compare(pairs, por, want, wpor, what if what is not None else len(recs))
    return pairs, want


# ---- wga_stat_pairs ---------------------------------------------------------------------------------------------------------------
def shaped(n, shape, k0=0):
    """n records of K33's mix of numbers as one pair (1), every record its own pair (0), or 2 / 3 pairs interleaved a, b, a, b, ..."""
    out = k33.some(n, k0)
    for k, r in enumerate(out):
        j = k if shape == 0 else k % shape
        r.update(rname=b"tgt%d" % j, qname=b"q.%d" % (j % 2 if shape else j), ref_size=3 * 10 ** 9 + (j % 3 if shape else j),
                 query_size=10 ** 9 + j)
    return out


def check_abi_record_counts(eng, ns=COUNTS):
    for n in ns:
        for shape in (1, 0, 2, 3):
            pairs, _ = check(eng, shaped(n, shape, n % 7), what=(n, shape))
            assert len(pairs) == (n if shape == 0 else min(n, shape))


def check_abi_key(eng):
    """pairs that differ in one part of the key only; empty names; a span outside d_names is the empty name"""
    base = dict(rname=b"chr1", qname=b"ctg7", ref_size=1000, query_size=900)
    variants = [dict(), dict(ref_size=1001), dict(query_size=901), dict(rname=b"chr2"), dict(qname=b"ctg8"), dict(rname=b"chr"),
                dict(qname=b"ctg77"), dict(rname=b"chr1c", qname=b"tg7"), dict(rname=b"chr1ctg", qname=b"7"), dict(rname=b"", qname=b"chr1ctg7"),
                dict(rname=b"chr1ctg7", qname=b""), dict(rname=b"", qname=b""), dict(rname=b"", qname=b"", ref_size=1001)]
    recs = []
    for rep in range(3):                                                          # every variant three times, interleaved
        for k, v in enumerate(variants):
            recs.append(rec(**dict(base, **v), ref_start=50 + 7 * k + rep, query_start=40 + k - rep, match=10 + k, inv_ev=rep % 2,
                            ins_bp=rep))
    pairs, _ = check(eng, recs)
    assert len(pairs) == len(variants) and all(int(p["n_recs"]) == 3 for p in pairs)
    # ("ab", "c") and ("a", "bc"): the same bytes back to back, two pairs
    pairs, _ = check(eng, [rec(rname=b"ab", qname=b"c"), rec(rname=b"a", qname=b"bc"), rec(rname=b"ab", qname=b"c")])
    assert [int(p["n_recs"]) for p in pairs] == [2, 1]
    # spans: one that reaches beyond d_names is the empty name and pairs with a record whose names are empty
    recs = [rec(rname=b"abcd", qname=b"efgh", ref_size=5, query_size=6, match=k + 1) for k in range(5)]
    total = 8 * 5
    recs[0]["spans"] = ((total - 2, 3), (0, total + 1))
    recs[1]["spans"] = ((total + 1, 0), (U64, 1))
    recs[2]["spans"] = ((total - 4, 4), (total, 0))                               # ends exactly at the buffer's end: "efgh", ""
    recs[3]["spans"] = ((U64 - 1, 0xFFFFFFFF), (5, 0xFFFFFFFF))
    names = [(b"", b""), (b"", b""), (b"efgh", b""), (b"", b""), (b"abcd", b"efgh")]
    pairs, _ = check(eng, recs, seen=[dict(r, rname=s[0], qname=s[1]) for r, s in zip(recs, names)])
    assert [int(p["n_recs"]) for p in pairs] == [3, 1, 1]


def random_recs(seed):
    """40 .. 740 records over a pool of about n / 6 keys whose parts repeat, with K33's wild counters"""
    rnd = random.Random(9100 + seed)
    n = 40 + (seed * 67) % 700
    big = (0, 1, 9, 10, 99, 12345, 10 ** 6, (1 << 24) + 1, (1 << 32) - 1, 1 << 32, 10 ** 12, (1 << 53) + 1, 10 ** 19 - 1, U64)
    keys = [(b"ref.chr%d" % rnd.randrange(9) if rnd.random() < 0.9 else b'odd"\t%d' % rnd.randrange(3), rnd.choice((10 ** 8, 10 ** 8 + 1, U64)),
             b"qry.ctg%d" % rnd.randrange(12), rnd.choice((7 * 10 ** 7, 5))) for _ in range(2 + n // 6)]
    recs = []
    for _ in range(n):
        wild = rnd.random() < 0.1
        c = {f: (rnd.choice(big) if wild else rnd.randrange(10 ** rnd.randrange(1, 8))) for f in ref.COUNT_FIELDS}
        if rnd.random() < 0.6:
            c["inv_ev"] = 0
        rn, rs, qn, qs = rnd.choice(keys)
        recs.append(rec(rname=rn, qname=qn, ref_size=rs, ref_start=rnd.choice((rnd.randrange(10 ** 9), rs, U64)), query_size=qs,
                        query_start=rnd.randrange(10 ** 9), c=c))
    return recs


def check_abi_random(eng, seeds):
    for seed in seeds:
        check(eng, random_recs(seed), what=("seed", seed))


def check_abi_collisions(eng, seeds):
    """stat_pair_hash_bits = 1: two start slots for all pairs, the bytes and sizes decide"""
    eng.set_param("stat_pair_hash_bits", 1)
    try:
        assert eng.get_param("stat_pair_hash_bits") == 1
        check_abi_random(eng, seeds)
        check_abi_key(eng)
    finally:
        eng.set_param("stat_pair_hash_bits", 64)
    assert eng.get_param("stat_pair_hash_bits") == 64
    for bad in (0, 65, -1):
        assert eng.lib.wga_ctx_set_param(eng.ctx, b"stat_pair_hash_bits", bad) == E_INVALID_ARG


def check_abi_wrapped(eng):
    """sums that wrap 2^64; a start above its size (the minimum stays the size); ref_size < aligned_size; aligned_size == 0"""
    recs = [rec(rname=b"w", ref_size=100, ref_start=500, query_size=80, query_start=90, match=U64, mismatch=U64 - 1, ins_bp=1 << 63),
            rec(rname=b"w", ref_size=100, ref_start=U64, query_size=80, query_start=81, match=5, mismatch=9, ins_bp=1 << 63, inv_ev=U64),
            rec(rname=b"w", ref_size=100, ref_start=100, query_size=80, query_start=80, match=1, inv_ev=1),
            rec(rname=b"small", ref_size=10, ref_start=3, query_size=10, query_start=4, match=25, del_bp=5),
            rec(rname=b"zero", ref_size=10, ref_start=0, query_size=10, query_start=0, ins_bp=7),
            rec(rname=b"small", ref_size=10, ref_start=2, query_size=10, query_start=9, match=1)]
    pairs, want = check(eng, recs)
    assert (int(pairs[0]["ref_start"]), int(pairs[0]["query_start"])) == (100, 80)
    assert int(pairs[0]["sum"]["match"]) == 5 and int(pairs[0]["sum"]["ins_bp"]) == 0 and int(pairs[0]["sum"]["inv_ev"]) == 0
    assert (int(pairs[1]["ref_start"]), int(pairs[1]["query_start"])) == (2, 4)
    rows = [ref.row_of(w).split(b"\t") for w in want]
    assert len(rows[1][7]) == 20 and rows[1][7] == b"%d" % ((10 - 31) & U64)       # ref_size < aligned_size: column 8 wraps
    assert rows[2][6] == b"0" and rows[2][8] == b"NaN" and rows[2][9] == b"NaN"
    check_rows(eng, want)


def fold_recs(n_a, big_at, all_inverted=False):
    """pair A's records (n_a of them, every second one inverted unless all are) interleaved with non-members: a second pair B whose
    records are inverted too.  A's inverted records are worth 1.0, but the one with index big_at among them is worth 2^24"""
    recs, k_inv = [], 0
    for k in range(n_a):
        inv = all_inverted or k % 2 == 0
        if inv:
            m = 1 << 24 if k_inv == big_at else 1
            k_inv += 1
        recs.append(rec(rname=b"A", qname=b"qa", ref_size=10 ** 9, query_size=10 ** 9, match=m if inv else 3 + k, inv_ev=1 if inv else 0))
        if k % 3 == 1:
            recs.append(rec(rname=b"B", qname=b"qb", ref_size=10 ** 9, query_size=10 ** 9, match=2 + k % 5, inv_ev=1 + k % 2))
    assert k_inv > big_at
    return recs, k_inv


def check_abi_fold_order(eng):
    """2^24, then many 1.0 stays 2^24 (2^24 + 1 is a tie that rounds to even); the reverse counts every 1.0.  The large value
    stands at the borders of the fold's loads of 64 (inverted record 63 / 64 of the pair) and of the sort's blocks (sorted place
    1023 / 1024)."""
    got = {}
    for big_at in (0, 1, 63, 64, 65, 149):
        recs, k_inv = fold_recs(300, big_at)
        assert k_inv == 150
        _, want = check(eng, recs, what=("fold", big_at))
        got[big_at] = float(want[0]["inv_size"])
    # j times 1.0 in front: 2^24 + j, a tie for an odd j; every 1.0 behind is a tie again and is lost where the mantissa is even
    assert got[0] == got[1] == float(1 << 24) and got[63] == got[64] == float((1 << 24) + 64) and got[149] == float((1 << 24) + 148), got
    for big_at in (1023, 1024):                                                   # all of A inverted: inverted index = sorted place
        recs, _ = fold_recs(1100, big_at, all_inverted=True)
        check(eng, recs, what=("fold", big_at))
    # inv_ev = 2^64 - 1: a division by zero, the sum is inf from there on
    recs, _ = fold_recs(200, 70)
    at = next(k for k in range(150, len(recs)) if recs[k]["rname"] == b"A" and recs[k]["c"]["inv_ev"])
    recs[at]["c"] = counts(match=9, inv_ev=U64)
    _, want = check(eng, recs, what="inf")
    assert np.isinf(want[0]["inv_size"])


def check_abi_fold_start(eng):
    """d_inv_in: the folds start from the caller's values; and a repeat of the second call with other values rewrites inv_size
    alone"""
    recs, _ = fold_recs(300, 70)
    n_pairs = 2
    starts = [np.array([ref.f32_bits(np.float32(v)) for v in vals], dtype=np.uint32)
              for vals in ((1 << 24, 0.5), (3.0, float(1 << 25)), (0.0, 1.0))]
    for inv_in in starts:
        pairs, want = check(eng, recs, inv_in=inv_in, what=("start", list(inv_in)))
        assert len(pairs) == n_pairs
    assert ref.pairs([tup(r) for r in recs], starts[0])[0][0]["inv_size"] != ref.pairs([tup(r) for r in recs], starts[1])[0][0]["inv_size"]
    # a pair without an inverted record keeps its start value
    plain = [rec(rname=b"p", match=4), rec(rname=b"p", match=5), rec(rname=b"i", match=6, inv_ev=1)]
    pairs, _ = check(eng, plain, inv_in=starts[1][::-1].copy())
    assert int(pairs[0]["inv_size_bits"]) == int(starts[1][1])
    # the repeat: same outputs, other start values; a field the first pass wrote is not written again
    a = k33.Arrays(eng, recs)
    work = eng.empty(int(eng.lib.wga_stat_pairs_work_bytes(a.n)), np.uint8)
    n, names, nb, heads, cnt = a.args()
    npairs = C.c_uint64(0)
    args = (eng.ctx, n, names.ptr, nb, heads.ptr, cnt.ptr, work.ptr, C.byref(npairs))
    assert eng.lib.wga_stat_pairs(*args, None, None, None, 0) == 0 and npairs.value == n_pairs
    d_pairs, d_por = eng.empty(n_pairs, STAT_PAIR_DTYPE), eng.empty(n, np.uint32)
    d_inv = eng.upload(starts[0])
    assert eng.lib.wga_stat_pairs(*args, d_por.ptr, d_inv.ptr, d_pairs.ptr, n_pairs) == 0
    eng.sync()
    first = d_pairs.numpy()
    want0, wpor = ref.pairs([tup(r) for r in recs], starts[0])
    compare(first, d_por.numpy(), want0, wpor, "first pass")
    marked = first.copy()
    marked["n_recs"][1] = 77                                                      # the caller's own mark
    eng.copy_into(d_pairs, marked)
    eng.copy_into(d_inv, starts[1])
    assert eng.lib.wga_stat_pairs(*args, d_por.ptr, d_inv.ptr, d_pairs.ptr, n_pairs) == 0
    eng.sync()
    again = d_pairs.numpy()
    assert int(again["n_recs"][1]) == 77, "the repeat rewrote more than inv_size"
    again["n_recs"][1] = first["n_recs"][1]
    compare(again, d_por.numpy(), ref.pairs([tup(r) for r in recs], starts[1])[0], wpor, "repeat")
    assert eng.lib.wga_stat_pairs(*args, d_por.ptr, None, d_pairs.ptr, n_pairs) == 0          # and back to +0.0
    eng.sync()
    again = d_pairs.numpy()
    again["n_recs"][1] = first["n_recs"][1]
    compare(again, d_por.numpy(), ref.pairs([tup(r) for r in recs])[0], wpor, "repeat from 0")
    # other outputs: everything is written
    d_pairs2 = eng.upload(np.zeros(n_pairs, dtype=STAT_PAIR_DTYPE))
    assert eng.lib.wga_stat_pairs(*args, d_por.ptr, d_inv.ptr, d_pairs2.ptr, n_pairs) == 0
    eng.sync()
    compare(d_pairs2.numpy(), d_por.numpy(), ref.pairs([tup(r) for r in recs], starts[1])[0], wpor, "other outputs")


def raw_pairs(eng, a, n=None, work=True, null=(), names_bytes=None, npairs=True, second=None, cap=None):
    """one call by hand: (rc, *n_pairs).  second = the first call's n_pairs: the second call, into fresh outputs"""
    d_work = eng.empty(max(int(eng.lib.wga_stat_pairs_work_bytes(a.n)), 16), np.uint8) if work is True else work
    npv = C.c_uint64(second if second is not None else 7)
    p = dict(names=a.d_names.ptr, heads=a.d_heads.ptr, counts=a.d_counts.ptr, por=None, pairs=None)
    if second is not None:
        out = (eng.upload(np.full(a.n + 64, GUARD32, dtype=np.uint32)), eng.upload(np.full(32 * (second + 2), GUARD32, dtype=np.uint32)))
        p["por"], p["pairs"] = out[0].ptr, out[1].ptr
    for k in null:
        p[k] = None
    rc = eng.lib.wga_stat_pairs(eng.ctx, a.n if n is None else n, p["names"], len(a.names) if names_bytes is None else names_bytes,
                                p["heads"], p["counts"], d_work.ptr if d_work else None, C.byref(npv) if npairs else None, p["por"],
                                None, p["pairs"], cap if cap is not None else second or 0)
    eng.sync()
    if second is not None and rc != 0:
        assert (out[0].numpy() == GUARD32).all() and (out[1].numpy() == GUARD32).all(), "a refused call wrote"
    return rc, npv.value


def check_abi_arguments(eng):
    recs = shaped(5, 2)
    a = k33.Arrays(eng, recs)
    assert raw_pairs(eng, a) == (0, 2)
    for n in (None, 0):                                                           # whatever the count
        assert raw_pairs(eng, a, work=None, n=n)[0] == E_INVALID_ARG and raw_pairs(eng, a, npairs=False, n=n)[0] == E_INVALID_ARG
    for null in ("names", "heads", "counts"):
        assert raw_pairs(eng, a, null=(null,))[0] == E_INVALID_ARG, null
        assert raw_pairs(eng, a, n=0, null=(null,)) == (0, 0), null
    assert raw_pairs(eng, a, null=("names",), names_bytes=0) == (0, 2)            # no name has a byte: the sizes alone decide
    assert raw_pairs(eng, a, n=0) == (0, 0)
    pairs, por = eng.stat_pairs(0, None, 0, None, None)
    assert len(pairs) == 0 and len(por) == 0
    # the second call: a capacity below the pairs, one output without the other, a count that is not the first call's
    work = eng.empty(int(eng.lib.wga_stat_pairs_work_bytes(a.n)), np.uint8)
    assert raw_pairs(eng, a, work=work) == (0, 2)
    assert raw_pairs(eng, a, work=work, second=2, cap=1)[0] == E_TOO_SMALL
    assert raw_pairs(eng, a, work=work, second=2, null=("por",))[0] == E_INVALID_ARG
    assert raw_pairs(eng, a, work=work, second=2, null=("pairs",))[0] == E_INVALID_ARG
    assert raw_pairs(eng, a, work=work, second=3, cap=3)[0] == E_INVALID_ARG
    assert raw_pairs(eng, a, work=work, second=2, cap=5) == (0, 2)
    # the documented formula
    for n in (0, 1, 8, 9, 5000, 1 << 20):
        m = 16
        while m < 2 * n:
            m <<= 1
        c = 256 * ((n + 1023) // 1024) + 1
        want = 8 * (8 + m + 2 * (n + 1) + c + n // 1024 + c // 1024 + 8) + 4 * (6 * n + 2)
        assert int(eng.lib.wga_stat_pairs_work_bytes(n)) == (want + 7) // 8 * 8, n


# ---- wga_stat_pair_rows --------------------------------------------------------------------------------------------------------------
class PairArrays(k33.Arrays):
    """wga_stat_pair_rows' arrays for the restatement's pairs: K33's arrays over the pairs' heads and sums, and the inv_size bits"""

    def __init__(self, eng, want):
        recs = [rec(rname=w["key"][0], qname=w["key"][2], ref_size=w["key"][1], ref_start=w["ref_start"], query_size=w["key"][3],
                    query_start=w["query_start"], c=w["sum"]) for w in want]
        super().__init__(eng, recs)
        self.inv = np.array([ref.f32_bits(w["inv_size"]) for w in want] + [0], dtype=np.uint32)
        self.d_inv = eng.upload(self.inv)

    def args(self):
        return super().args() + (self.d_inv,)


def some_pairs(n, k0=0):
    """n pairs of K33's mix of numbers, every one the sum of two records"""
    recs = []
    for r in shaped(n, 0, k0):
        recs += [r, dict(r, ref_start=r["ref_start"] // 2, c=dict(r["c"], match=r["c"]["match"] + 1, inv_ev=1))]
    want, _ = ref.pairs([tup(r) for r in recs])
    assert len(want) == n
    return want


def check_rows(eng, want, shift=0):
    a = PairArrays(eng, want)
    rows = [ref.row_of(w) for w in want]
    text, row_off = eng.stat_pair_rows(*a.args(), out_shift=shift)
    exp = b"".join(rows)
    assert text == exp, (len(want), shift, first_difference(text, exp))
    assert [int(v) for v in row_off] == list(np.cumsum([0] + [len(r) for r in rows])), (len(want), shift)
    return text


def check_rows_record_counts(eng, ns=COUNTS):
    for n in ns:
        check_rows(eng, some_pairs(n, n % 5), shift=n % 16)


def check_rows_columns(eng):
    """column 8 and the f32 columns by hand"""
    want, _ = ref.pairs([tup(r) for r in (rec(rname=b"t\tab", ref_size=1000, ref_start=7, query_start=9, match=600, mismatch=150, inv_ev=1),
                                          rec(rname=b"t\tab", ref_size=1000, ref_start=5, query_start=11, match=150, del_bp=100, inv_ev=1),
                                          rec(rname=b"", qname=b"", ref_size=0, query_size=0))])
    text = check_rows(eng, want)
    rows = [ln.split(b"\t") for ln in text.split(b"\n")[:-1]]
    assert rows[0][:2] == [b'"t', b'ab"'] and rows[0][2:11] == [b"1000", b"5", b"qchr", b"1000000000", b"9", b"1000", b"0", b"0.75", b"0.9"]
    assert rows[0][18] == b"950.0"                                                # (750 + 750) / 2 + (250 + 150) / 2
    assert rows[1][:10] == [b"", b"0", b"0", b"", b"0", b"0", b"0", b"0", b"NaN", b"NaN"] and rows[1][17] == b"0.0"


def raw_rows(eng, a, n=None, work=True, null=(), names_bytes=None, total=True):
    d_work = eng.empty(max(int(eng.lib.wga_stat_rows_work_bytes(a.n)), 16), np.uint8)
    row_off = eng.empty(a.n + 2, np.uint64)
    tot = C.c_uint64(7)
    p = dict(names=a.d_names.ptr, heads=a.d_heads.ptr, sums=a.d_counts.ptr, inv=a.d_inv.ptr, row_off=row_off.ptr)
    for k in null:
        p[k] = None
    rc = eng.lib.wga_stat_pair_rows(eng.ctx, a.n if n is None else n, p["names"], len(a.names) if names_bytes is None else names_bytes,
                                    p["heads"], p["sums"], p["inv"], d_work.ptr if work else None, p["row_off"],
                                    C.byref(tot) if total else None, None)
    return rc, tot.value


def check_rows_arguments(eng):
    want = some_pairs(3)
    a = PairArrays(eng, want)
    exp = b"".join(ref.row_of(w) for w in want)
    assert raw_rows(eng, a) == (0, len(exp))
    for n in (None, 0):
        assert raw_rows(eng, a, work=False, n=n)[0] == E_INVALID_ARG and raw_rows(eng, a, total=False, n=n)[0] == E_INVALID_ARG
    for null in ("names", "heads", "sums", "inv", "row_off"):
        assert raw_rows(eng, a, null=(null,))[0] == E_INVALID_ARG, null
        assert raw_rows(eng, a, n=0, null=(null,)) == (0, 0), null
    assert raw_rows(eng, a, n=0) == (0, 0)
    assert eng.stat_pair_rows(0, None, 0, None, None, None)[0] == b""


class RawRows(k33.Raw):
    def call(self, out_ptr, total=None):
        n, names, nb, heads, cnt, inv = self.a.args()
        tot = C.c_uint64(total if total is not None else self.total if self.total is not None else 7)
        rc = self.eng.lib.wga_stat_pair_rows(self.eng.ctx, n, names.ptr, nb, heads.ptr, cnt.ptr, inv.ptr, self.work.ptr,
                                             self.row_off.ptr, C.byref(tot), out_ptr)
        self.eng.sync()
        assert rc == 0
        assert (self.row_off.numpy()[self.a.n + 1:] == 0xA5A5A5A5A5A5A5A5).all(), "a word behind d_row_off[n]"
        return int(tot.value)


def item_stream(eng):
    """600 rows, three blocks of the fill, behind their count call (as K33's item_stream)"""
    want = some_pairs(600, 3)
    a = PairArrays(eng, want)
    x = RawRows(eng, a)
    exp = b"".join(ref.row_of(w) for w in want)
    assert x.count(len(exp)) == len(exp)

    def fill(total_bytes, d_out):
        assert x.call(d_out, total=total_bytes) == total_bytes
    return ti.Stream(eng, x.row_off, 0, 600, exp, fill)


def check_rows_fill_short_total(eng):
    ti.check_short_total(item_stream(eng))


def check_rows_fill_scan_one_off(eng):
    ti.check_scan_one_off(item_stream(eng), size_checked=True)


# ---- the command -------------------------------------------------------------------------------------------------------------------
def three_ways(cli, *args, want=None, env=None, to=None, gz=False):
    """the command on its device path and under WGA_STAT_WRITER=host: the same bytes (of stdout, or of the file `to` that -o names),
    exit status and message; under WGA_TIMING=1 a run that counted a piece names the path that ran; and, where `want` is given,
    the restatement's bytes"""
    env = env or {}
    args = list(args) + (["-o", to, "-r"] if to else [])
    res = []
    for e in (env, dict(env, **HOST_WRITER)):
        rc, out, msg, timing = m2p.timed(cli, args, e)
        if to:
            out = open(to, "rb").read()
            out = gzip.decompress(out) if gz and out else out
        res.append((rc, out, msg, timing))
    dev, host = res
    assert dev[0] in (0, 1) and dev[:3] == host[:3], (args, dev[0], host[0], dev[2], host[2], first_difference(dev[1], host[1]))
    assert "stat table (host)" not in dev[3] and "stat table (device)" not in host[3], (dev[3], host[3])
    if dev[0] == 0:
        assert "stat table (host)" in host[3], host[3]
        if dev[1]:
            assert "stat table (device)" in dev[3], dev[3]
    if want is not None:
        assert dev[1] == want, (args, first_difference(dev[1], want))
    return dev[:3]


def paf_records(text):
    """the restatement's records of a PAF text, counters from the oracle"""
    out = []
    for ln in text.split(b"\n"):
        f = ln.split(b"\t")
        if len(f) < 12:
            continue
        cg = next(x for x in f[12:] if x.startswith(b"cg:Z:"))
        c = orc.parse_paf_to_cigar(cg.decode(), f[4] == b"-")
        out.append((f[5], int(f[6]), int(f[7]), f[0], int(f[1]), int(f[2]), c))
    return out


def maf_records(text):
    """the restatement's records of a MAF text: a block's first s-line against its second, counters from the oracle"""
    out = []
    for block in text.split(b"\na")[1:]:
        s = [ln.split() for ln in block.split(b"\n") if ln[:2] in (b"s ", b"s\t")]
        if len(s) < 2:
            continue
        t, q = s[0], s[1]
        neg = q[4] == b"-"
        c, _ = orc.parse_maf_seq_to_cigar(t[6], q[6], neg)
        qstart, qali, qsize = int(q[2]), int(q[3]), int(q[5])
        out.append((t[1], int(t[5]), int(t[2]), q[1], qsize, qsize - qstart - qali if neg else qstart, c))
    return out


def check_cli_fixtures(cli):
    maf = os.path.join(GOLDEN, "test.maf")
    want = ref.table(maf_records(b"\n" + open(maf, "rb").read()))
    assert want.count(b"\n") >= 2
    assert three_ways(cli, "stat", maf, want=want) == (0, want, "")
    paf = os.path.join(GOLDEN, "testdotplot.paf")
    want = ref.table(paf_records(open(paf, "rb").read()))
    assert want.count(b"\n") >= 2
    assert three_ways(cli, "stat", "-f", "paf", paf, want=want) == (0, want, "")


TARGETS = (b"c 1", b"c1", b"c10")


def paf_case(seed, n):
    """n records over three targets x three queries, `-` records (inverted) throughout: (the text, the restatement's records)"""
    rnd = random.Random(9700 + seed)
    lines = []
    for k in range(n):
        cg = k33.random_cigar(rnd)
        neg = rnd.random() < 0.5
        t, q = TARGETS[k % 3], (b"q1", b"qry.2", b"q")[(k // 3) % 3]
        tl, ql = 10 ** 8 + (k % 3), 10 ** 7 + (k // 3) % 3 + (1 if k % 37 == 36 else 0)    # now and then an equal name pair of another size
        ts, qs = rnd.randrange(10 ** 7), rnd.randrange(10 ** 6)
        lines.append(b"%s\t%d\t%d\t%d\t%s\t%s\t%d\t%d\t%d\t10\t20\t60\tcg:Z:%s\n" % (q, ql, qs, qs + 50, b"-" if neg else b"+", t, tl, ts,
                                                                                   ts + 50, cg.encode()))
    text = b"".join(lines)
    return text, paf_records(text)


def check_cli_paf(cli, tmp_path):
    text, records = paf_case(1, 300)
    paf = write(tmp_path, "a.paf", text)
    want = ref.table(records)
    first = [ln.split(b"\t")[0] for ln in want.split(b"\n")[1:-1]]
    assert len(first) >= 9 and set(first[:first.index(b"c10")]) == {b"c 1", b"c1"} and first[0] == b"c 1" and first[1] == b"c1"
    assert three_ways(cli, "stat", "-f", "paf", paf, want=want) == (0, want, "")
    # five pieces: every pair spans them, with inverted records in each, so the folds carry over
    chunk = len(text) // 5
    at, pieces_with_inv = 0, set()
    for ln in text.split(b"\n")[:-1]:                                             # the pieces that hold a `-` record of the first pair
        f = ln.split(b"\t")
        if (f[5], f[0], f[4]) == (b"c 1", b"q1", b"-"):
            pieces_with_inv.add(at // chunk)
        at += len(ln) + 1
    assert len(pieces_with_inv) >= 3 and len(text) // chunk >= 4
    assert three_ways(cli, "stat", "-f", "paf", paf, want=want, env={"WGA_CHUNK_BYTES": str(chunk)}) == (0, want, "")
    assert three_ways(cli, "stat", "-f", "paf", paf, want=want, env={"WGA_PAF_READER": "host"}) == (0, want, "")
    assert three_ways(cli, "stat", "-f", "paf", paf, want=want, to=str(tmp_path / "x.gz"), gz=True) == (0, want, "")
    # the fold across pieces is a fold, not a sum of sums: the order shows
    big = b"q\t900\t0\t50\t-\tT\t1000\t0\t50\t10\t20\t60\tcg:Z:16777216M\n"
    one = b"q\t900\t0\t50\t-\tT\t1000\t0\t50\t10\t20\t60\tcg:Z:1M\n"
    for name, body in (("f.paf", big + one * 40), ("r.paf", one * 40 + big)):
        path = write(tmp_path, name, body)
        want = ref.table(paf_records(body))
        assert three_ways(cli, "stat", "-f", "paf", path, want=want, env={"WGA_CHUNK_BYTES": str(len(body) // 6)})[0] == 0
    assert b"\t16777216.0\t" in ref.table(paf_records(big + one * 40)) and b"\t16777256.0\t" in ref.table(paf_records(one * 40 + big))


def check_cli_empty_and_errors(cli, tmp_path):
    assert three_ways(cli, "stat", "-f", "paf", write(tmp_path, "e.paf", b""), want=b"") == (0, b"", "")
    assert three_ways(cli, "stat", write(tmp_path, "e.maf", b"##maf version=1\n\n"), want=b"") == (0, b"", "")
    text, _ = paf_case(4, 60)
    lines = text.split(b"\n")[:-1]
    lines[-3] += b"3N"
    bad = write(tmp_path, "b.paf", b"\n".join(lines) + b"\n")
    to = write(tmp_path, "b.tsv", b"")
    assert three_ways(cli, "stat", "-f", "paf", bad, env={"WGA_CHUNK_BYTES": str(len(text) // 4)}) == (1, b"", "CIGAR OP `N` invalid")
    assert three_ways(cli, "stat", "-f", "paf", bad, to=to) == (1, b"", "CIGAR OP `N` invalid")


def maf_case(seed, n):
    """n MAF blocks of a target, a query and a second query, over three targets x three queries whose sizes go with their names:
    (the file's text, the restatement's records for the first query, ... for the second).  A MAF name cannot hold the white space
    that makes two names equal under natord, so the targets here only sort out of their first-appearance order"""
    rnd = random.Random(9800 + seed)
    out, recs1, recs2 = [b"##maf version=1 scoring=none\n\n"], [], []

    def rows(cols):
        t, q = bytearray(), bytearray()
        for _ in range(cols):
            x = rnd.random()
            t.append(45 if x < 0.08 else k33.BASES[rnd.randrange(10)])
            q.append(45 if 0.08 <= x < 0.16 else (t[-1] if x < 0.8 and t[-1] != 45 else k33.BASES[rnd.randrange(10)]))
        return bytes(t), bytes(q)

    for k in range(n):
        cols = rnd.choice((1, 7, 60, 200, 333))
        t, q = rows(cols)
        _, q2 = rows(cols)
        tn = (b"c2", b"c1", b"c10")[k % 3]
        tsize, tstart, tali = 10 ** 8 + k % 3, rnd.randrange(10 ** 7), cols - t.count(b"-")
        out.append(b"a score=%d\ns %s %d %d + %d %s\n" % (k, tn, tstart, tali, tsize, t))
        for name, qsize, row, into in ((b"qA.%d" % ((k // 3) % 3), 10 ** 7 + (k // 3) % 3, q, recs1), (b"qB", 10 ** 7, q2, recs2)):
            neg = rnd.random() < 0.5
            qstart, qali = rnd.randrange(10 ** 6), cols - row.count(b"-")
            out.append(b"s %s %d %d %s %d %s\n" % (name, qstart, qali, b"-" if neg else b"+", qsize, row))
            c, _ = orc.parse_maf_seq_to_cigar(t, row, neg)
            into.append((tn, tsize, tstart, name, qsize, qsize - qstart - qali if neg else qstart, c))
        out.append(b"\n")
    return b"".join(out), recs1, recs2


def check_cli_maf(cli, tmp_path):
    text, recs1, recs2 = maf_case(3, 200)
    maf = write(tmp_path, "a.maf", text)
    want1, want2 = ref.table(recs1), ref.table(recs2)
    assert want1.count(b"\n") == 1 + 9 and want2.count(b"\n") == 1 + 3
    assert three_ways(cli, "stat", maf, want=want1) == (0, want1, "")
    assert three_ways(cli, "stat", "-q", "qB", maf, want=want2) == (0, want2, "")             # the named query of a multi-query file
    env = {"WGA_CHUNK_BYTES": str(len(text) // 5)}
    assert three_ways(cli, "stat", maf, want=want1, env=env, to=str(tmp_path / "m.tsv.gz"), gz=True) == (0, want1, "")
    assert three_ways(cli, "stat", "-q", "qB", maf, want=want2, env=dict(env, WGA_MAF_READER="host")) == (0, want2, "")


def check_cli_gpus(cli, tmp_path, gpus=2):
    """--gpus N: the counters meet on the host and device 0 builds the table — the bytes of one device, also for a failing file"""
    text, records = paf_case(5, 120)
    paf = write(tmp_path, "g.paf", text)
    want = ref.table(records)
    g = ("--gpus", str(gpus))
    for env in ({"WGA_CHUNK_BYTES": str(len(text) // 3)}, {"WGA_PAF_READER": "host"}):
        assert three_ways(cli, *g, "stat", "-f", "paf", paf, want=want, env=env) == (0, want, ""), env
    lines = text.split(b"\n")[:-1]
    lines[50] += b"3N"
    bad = write(tmp_path, "gb.paf", b"\n".join(lines) + b"\n")
    assert three_ways(cli, *g, "stat", "-f", "paf", bad) == (1, b"", "CIGAR OP `N` invalid")
    mtext, recs1, recs2 = maf_case(2, 60)
    maf = write(tmp_path, "g.maf", mtext)
    assert three_ways(cli, *g, "stat", maf, want=ref.table(recs1), env={"WGA_CHUNK_BYTES": str(len(mtext) // 3)})[0] == 0
    assert three_ways(cli, *g, "stat", "-q", "qB", maf, want=ref.table(recs2), env={"WGA_MAF_READER": "host"})[0] == 0
