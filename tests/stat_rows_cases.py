"""The TSV rows of `stat --each` on the device (K33): the C-ABI entries (Engine.stat_rows, Engine.f32_text) against stat_rows_ref
(the restatement from stat.rs, numpy.float32 and Dragon4), and the command with its device writer against WGA_STAT_WRITER=host and
the restatement over the oracle's counters.
Imported by test_emu_stat_rows.py (emulator build, CPU) and test_gpu_stat_rows.py (the product on a GPU); each provides the
`cli` and `eng` fixtures."""
import ctypes as C
import functools
import gzip
import random

import numpy as np

import maf2paf_cases as m2p
import oracle_py as orc
import stat_rows_ref as ref
import text_items_cases as ti
from chain_split_cases import run, write
from wgatools_amd.engine import COUNTS_DTYPE, STAT_ROW_HEAD_DTYPE

U64 = (1 << 64) - 1
E_INVALID_ARG = -1
COUNTS = (0, 1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2049)            # the wave, block and scan-partial borders
WIDTHS = (0, 1 << 32, 10 ** 19 - 1, U64)                                       # 1, 10, 19 and 20 digits
HOST_WRITER = {"WGA_STAT_WRITER": "host"}


# ---- records and arrays ----------------------------------------------------------------------------------------------------------
def counts(**kw):
    c = dict.fromkeys(ref.COUNT_FIELDS, 0)
    c.update(kw)
    return c


def rec(rname=b"tchr", qname=b"qchr", ref_size=10 ** 9, ref_start=100, query_size=10 ** 9, query_start=700, c=None, **kw):
    return dict(rname=rname, qname=qname, ref_size=ref_size, ref_start=ref_start, query_size=query_size, query_start=query_start,
                c=c if c is not None else counts(**kw))


def some(n, k0=0):
    """n records with names and numbers of several widths and all three floats in several layouts"""
    out = []
    for k in range(k0, k0 + n):
        m = 10 ** (k % 9) + 3 * k
        out.append(rec(rname=b"t" * (1 + k % 5), qname=b"q%d" % (k % 11), ref_size=2 * 10 ** 9 + k, ref_start=10 ** (k % 7),
                       query_size=10 ** 9 + k, query_start=7 * k,
                       c=counts(match=m, mismatch=k % 13, ins_ev=k % 3, ins_bp=(k % 3) * 17, del_ev=k % 4, del_bp=(k % 4) * 5,
                                inv_ev=k % 5 // 4, inv_ins_ev=k % 2, inv_ins_bp=k % 7, inv_del_ev=k % 3 // 2, inv_del_bp=k % 11)))
    return out


def want_rows(recs):
    return [ref.row(r["rname"], r["ref_size"], r["ref_start"], r["qname"], r["query_size"], r["query_start"], r["c"]) for r in recs]


class Arrays:
    """wga_stat_rows' arrays for a list of records: the names back to back in one buffer (16 bytes of slack behind), one head
    and one set of counters per record.  A record's `spans` = ((rname_off, rname_len), (qname_off, qname_len)) replaces its own."""

    def __init__(self, eng, recs):
        self.eng, self.recs, self.n = eng, recs, len(recs)
        names = bytearray()
        heads = np.zeros(self.n + 1, dtype=STAT_ROW_HEAD_DTYPE)
        cnt = np.zeros(self.n + 1, dtype=COUNTS_DTYPE)
        for k, r in enumerate(recs):
            h = heads[k]
            for f in ("ref_size", "ref_start", "query_size", "query_start"):
                h[f] = r[f]
            h["rname_off"], h["rname_len"] = len(names), len(r["rname"])
            names += r["rname"]
            h["qname_off"], h["qname_len"] = len(names), len(r["qname"])
            names += r["qname"]
            for f in ref.COUNT_FIELDS:
                cnt[k][f] = r["c"][f]
        self.names = bytes(names)
        for k, r in enumerate(recs):
            if "spans" in r:
                (heads[k]["rname_off"], heads[k]["rname_len"]), (heads[k]["qname_off"], heads[k]["qname_len"]) = r["spans"]
        self.heads, self.counts = heads, cnt
        self.d_names = eng.upload(np.frombuffer(self.names + b"\0" * 16, dtype=np.uint8))
        self.d_heads, self.d_counts = eng.upload(heads), eng.upload(cnt)

    def args(self):
        return self.n, self.d_names, len(self.names), self.d_heads, self.d_counts


def check(eng, recs, want=None, shift=0):
    """both calls (Engine.stat_rows checks the guards around the text and that the total stays): the text is the restatement's
    rows in input order, and row_off their prefix sums"""
    a = Arrays(eng, recs)
    rows = want if want is not None else want_rows(recs)
    text, row_off = eng.stat_rows(*a.args(), out_shift=shift)
    exp = b"".join(rows)
    assert text == exp, (len(recs), shift, first_difference(text, exp))
    assert [int(v) for v in row_off] == list(np.cumsum([0] + [len(r) for r in rows])), (len(recs), shift)
    return text


def first_difference(got, exp):
    k = next((i for i, (x, y) in enumerate(zip(got, exp)) if x != y), min(len(got), len(exp)))
    return len(got), len(exp), k, got[max(0, k - 60):k + 60], exp[max(0, k - 60):k + 60]


# ---- the C-ABI entry ---------------------------------------------------------------------------------------------------------------
def check_abi_record_counts(eng, ns=COUNTS):
    for n in ns:
        check(eng, some(n, n % 7))


class Raw:
    """the two calls by hand with guards around everything a call writes: 8 words behind row_off's n + 1, 64 bytes around d_out"""
    GUARD = 64

    def __init__(self, eng, a, work=None):
        self.eng, self.a = eng, a
        self.work = work if work is not None else eng.empty(max(int(eng.lib.wga_stat_rows_work_bytes(a.n)), 16), np.uint8)
        self.row_off = eng.upload(np.full(a.n + 1 + 8, 0xA5A5A5A5A5A5A5A5, dtype=np.uint64))
        self.total = None

    def call(self, out_ptr, total=None):
        n, names, nb, heads, cnt = self.a.args()
        tot = C.c_uint64(total if total is not None else self.total if self.total is not None else 7)
        rc = self.eng.lib.wga_stat_rows(self.eng.ctx, n, names.ptr, nb, heads.ptr, cnt.ptr, self.work.ptr, self.row_off.ptr,
                                        C.byref(tot), out_ptr)
        self.eng.sync()
        assert rc == 0
        off = self.row_off.numpy()
        assert (off[self.a.n + 1:] == 0xA5A5A5A5A5A5A5A5).all(), "a word behind d_row_off[n]"
        return int(tot.value)

    def count(self, room):
        """the count call; the output buffer (room bytes for the text) is there already and must stay as it is"""
        self.out = self.eng.upload(np.full(room + 2 * self.GUARD + 32, 0xA5, dtype=np.uint8))
        self.total = self.call(None)
        assert (self.out.numpy() == 0xA5).all()
        return self.total

    def fill(self, shift=0):
        assert self.call(self.out.ptr + self.GUARD + shift) == self.total
        got = self.out.numpy()
        lead = self.GUARD + shift
        assert (got[:lead] == 0xA5).all() and (got[lead + self.total:] == 0xA5).all(), "a byte outside d_out[0 .. total)"
        return got[lead:lead + self.total].tobytes()


def check_abi_alignment(eng):
    """d_out at every offset 0 .. 15 of a buffer: the guards in front of and behind the text stay as they were after the count
    call and after the fill; the same arguments for both calls"""
    for n in (1, 3, 257):
        recs = some(n, 2)
        a = Arrays(eng, recs)
        exp = b"".join(want_rows(recs))
        for shift in range(16):
            x = Raw(eng, a)
            assert x.count(len(exp)) == len(exp)
            assert [int(v) for v in x.row_off.numpy()[:n + 1]] == list(np.cumsum([0] + [len(r) for r in want_rows(recs)]))
            assert x.fill(shift) == exp, (n, shift)


def check_abi_numbers(eng):
    """every integer column at 1, 10, 19 and 20 digits"""
    recs = []
    for k, w in enumerate(WIDTHS):
        v = WIDTHS[k:] + WIDTHS[:k]
        recs.append(rec(ref_size=w, ref_start=v[1], query_size=v[2], query_start=v[3],
                        c=dict(zip(ref.COUNT_FIELDS, (v[(k + j) % 4] for j in range(11))))))
        recs.append(rec(ref_size=w, ref_start=w, query_size=w, query_start=w, c=dict.fromkeys(ref.COUNT_FIELDS, w)))
    text = check(eng, recs)
    assert b"\t18446744073709551615\t" in text and b"\t9999999999999999999\t" in text and b"\t4294967296\t" in text


def check_abi_wrapped_sums(eng):
    recs = [rec(match=5, mismatch=U64 - 4),                                       # aligned_size wraps to 0 with match > 0
            rec(match=1 << 63, del_bp=1 << 63),
            rec(match=10, inv_ev=U64, ins_bp=3),                                  # inv_ev + 1 wraps to 0
            rec(match=U64, mismatch=U64, del_bp=U64, inv_del_bp=U64, ins_bp=U64, inv_ins_bp=U64, inv_ev=2)]
    rows = want_rows(recs)
    cols = [r.split(b"\t") for r in rows]
    assert cols[0][6] == b"0" and cols[0][8] == b"inf" and cols[0][9] == b"NaN"   # (5 + 2^64 - 4) wraps to 1... over 0
    assert cols[1][6] == b"0" and cols[1][8] == b"inf"
    assert cols[2][17] == b"inf"
    check(eng, recs, rows)


def check_abi_names(eng):
    long300, long8k = bytes(65 + k % 26 for k in range(300)), bytes(97 + k % 26 for k in range(8192))
    recs = [rec(rname=b"", qname=b""), rec(rname=b"a", qname=b"b"), rec(rname=long300, qname=long300[::-1]),
            rec(rname=b"t\tab", qname=b'q"uote"'), rec(rname=b"c\rr", qname=b"l\nf"), rec(rname=b'"', qname=b'""\t""'),
            rec(rname=b"plain name", qname=b"comma,semi;")]
    rows = want_rows(recs)
    assert rows[3].startswith(b'"t\tab"\t') and b'\t"q""uote"""\t' in rows[3] and rows[5].startswith(b'""""\t')
    check(eng, recs, rows)
    # a span that reaches beyond d_names is an empty name; one that ends exactly at its end is not
    recs = [rec(rname=b"abcd", qname=b"efgh") for _ in range(4)]
    total = 8 * 4
    recs[0]["spans"] = ((total - 2, 3), (0, total + 1))
    recs[1]["spans"] = ((total + 1, 0), (U64, 1))
    recs[2]["spans"] = ((total - 4, 4), (total, 0))
    recs[3]["spans"] = ((U64 - 1, 0xFFFFFFFF), (5, 0xFFFFFFFF))
    seen = [(b"", b""), (b"", b""), (b"efgh", b""), (b"", b"")]
    rows = want_rows([dict(r, rname=s[0], qname=s[1]) for r, s in zip(recs, seen)])
    check(eng, recs, rows)
    # one name of 8 KiB: its block's stretch is longer than the stage and is written directly, the blocks around it staged
    for at in (0, 255, 256, 300):
        recs = some(600, 1)
        recs[at] = rec(rname=long8k, qname=b"q", match=3)
        check(eng, recs)
    recs = some(40)
    recs[7] = rec(rname=b"r", qname=b'x"' + long8k + b"\t")
    check(eng, recs, shift=5)


def check_abi_floats(eng):
    """the three f32 columns through the counters"""
    cases = [
        (counts(), (b"NaN", b"NaN", b"0.0")),                                     # aligned_size 0
        (counts(match=77), (b"1.0", b"1.0", b"0.0")),
        (counts(match=1, mismatch=2), (b"0.33333334", b"1.0", b"0.0")),
        (counts(match=2, del_bp=1), (b"0.6666667", b"0.6666667", b"0.0")),
        (counts(match=1, mismatch=1, del_bp=8), (b"0.1", b"0.2", b"0.0")),
        (counts(match=(1 << 24) + 1, del_bp=(1 << 24) - 1), (b"0.5", None, b"0.0")),    # 2^24 + 1 -> 2^24: a tie, to even
        (counts(match=(1 << 24) + 3, del_bp=(1 << 24) - 3), (b"0.5000001", None, b"0.0")),  # ... and up to 2^24 + 4
        (counts(match=(1 << 53) + 1, mismatch=1, del_bp=5), None),
        (counts(match=U64, inv_ev=1, ins_bp=1), None),                            # operands of 2^64 - 1
        (counts(match=U64 - 1, mismatch=1), None),
        (counts(match=10, inv_ev=1), (b"1.0", b"1.0", b"10.0")),
        (counts(match=10, inv_ev=1, ins_bp=1), (b"1.0", b"1.0", b"10.5")),
        (counts(match=5 * 10 ** 12, inv_ev=1), (b"1.0", b"1.0", b"5000000000000.0")),   # kk = 13: still plain
        (counts(match=10 ** 13, inv_ev=1), (b"1.0", b"1.0", b"1e13")),
        (counts(match=10 ** 13 + 10 ** 9, inv_ev=1), (b"1.0", b"1.0", b"1.0001e13")),
        (counts(match=1 << 62, inv_ev=1), (b"1.0", b"1.0", b"4.611686e18")),
        (counts(match=1, del_bp=10 ** 6), (b"9.99999e-7", None, b"0.0")),
        (counts(match=1, del_bp=99999), (b"0.00001", None, b"0.0")),
        (counts(match=1, del_bp=U64 - 1), (b"5.421011e-20", None, b"0.0")),
        (counts(match=3, inv_ev=2), (b"1.0", b"1.0", b"2.0")),
    ]
    recs = [rec(c=c) for c, _ in cases]
    rows = want_rows(recs)
    for row, (c, exp) in zip(rows, cases):
        col = row.split(b"\t")
        if exp:
            for at, e in zip((8, 9, 17), exp):
                assert e is None or col[at] == e, (c, at, col[at], e)
    check(eng, recs, rows)


LAYOUT_BITS = (0x3727C5AC, 0x3727C5AB, 0x551184E7, 0x551184E6, 0x4B18967F, 0x4B189680)   # 1e-5, 9.999999e-6, 1e13, 9.999999e12, 9999999.0, 1e7
EDGE_BITS = (0x00000000, 0x80000000, 0x00000001, 0x007FFFFF, 0x00800000, 0x3F800000, 0x3DCCCCCD, 0x3EAAAAAB, 0x7F7FFFFF, 0x7F800000,
             0xFF800000, 0x7FC00000, 0x7F800001, 0xFFFFFFFF)


@functools.lru_cache(maxsize=None)
def f32_patterns():
    """(the patterns, the restatement's texts): the named ones, the neighbours of mantissa-0 values, the layout borders, a negative
    value of each layout, and 2^20 patterns from a fixed seed.  Computed once and shared."""
    bits = list(EDGE_BITS)
    for b in (0x4B800000, 0x4B000000, 0x3F000000, 0x00800000):                    # a mantissa of 0: the lower neighbour is closer
        bits += [b - 1, b, b + 1]
    for b in LAYOUT_BITS + (0x358637BD,):                                         # ... and 1e-6, where the exponent form begins
        bits += [b - 1, b, b + 1]
    bits += [0x80000000 | b for b in (0x42F6E979, 0x3DFCD680, 0x3727C5AC, 0x551184E7, 0x4B18967F, 0x1E3CE508, 0x7149F2CA, 0x00000001)]
    rnd = np.random.RandomState(20261020)
    bits = np.concatenate([np.array(bits, dtype=np.uint32), rnd.randint(0, 1 << 32, size=1 << 20, dtype=np.uint64).astype(np.uint32)])
    return bits, ref.f32_texts(bits)


def check_ref_layouts():
    """the restatement prints the named values as ryu does (the pretty::format32 cases, by hand)"""
    t = ref.f32_text_of_bits
    assert [t(b) for b in EDGE_BITS[:12]] == [b"0.0", b"-0.0", b"1e-45", b"1.1754942e-38", b"1.1754944e-38", b"1.0", b"0.1",
                                               b"0.33333334", b"3.4028235e38", b"inf", b"-inf", b"NaN"]
    assert [t(b) for b in LAYOUT_BITS] == [b"0.00001", b"0.000009999999", b"1e13", b"9999999000000.0", b"9999999.0", b"10000000.0"]
    assert t(0x358637BD) == b"0.000001" and t(0x358637BC) == b"9.999999e-7"           # the border between 0.00000d and d e-7
    assert t(0x4B800000) == b"16777216.0" and t(0x4B7FFFFF) == b"16777215.0" and t(0x4B800001) == b"16777218.0"
    assert t(0xC2F6E979) == b"-123.456" and t(0x9E3CE508) == b"-1e-20" and t(0xF149F2CA) == b"-1e30"


def check_f32_text(eng):
    bits, want = f32_patterns()
    got = eng.f32_text(bits)
    bad = [(hex(int(b)), g, w) for b, g, w in zip(bits, got, want) if g != w]
    assert not bad, (len(bad), bad[:10])
    assert eng.f32_text(np.zeros(0, dtype=np.uint32)) == []


def raw(eng, a, n=None, work=True, null=(), names_bytes=None, total=True):
    d_work = eng.empty(max(int(eng.lib.wga_stat_rows_work_bytes(a.n)), 16), np.uint8)
    row_off = eng.empty(a.n + 2, np.uint64)
    tot = C.c_uint64(7)
    p = dict(names=a.d_names.ptr, heads=a.d_heads.ptr, counts=a.d_counts.ptr, row_off=row_off.ptr)
    for k in null:
        p[k] = None
    rc = eng.lib.wga_stat_rows(eng.ctx, a.n if n is None else n, p["names"], len(a.names) if names_bytes is None else names_bytes,
                               p["heads"], p["counts"], d_work.ptr if work else None, p["row_off"], C.byref(tot) if total else None, None)
    return rc, tot.value


def check_abi_arguments(eng):
    recs = some(3)
    a = Arrays(eng, recs)
    want = b"".join(want_rows(recs))
    assert raw(eng, a) == (0, len(want))
    for n in (None, 0):                                                           # whatever the count
        assert raw(eng, a, work=False, n=n)[0] == E_INVALID_ARG and raw(eng, a, total=False, n=n)[0] == E_INVALID_ARG
    for null in ("names", "heads", "counts", "row_off"):
        assert raw(eng, a, null=(null,))[0] == E_INVALID_ARG, null
        assert raw(eng, a, n=0, null=(null,)) == (0, 0), null
    assert raw(eng, a, null=("names",), names_bytes=0) == (0, len(b"".join(want_rows([dict(r, rname=b"", qname=b"") for r in recs]))))
    assert raw(eng, a, n=0) == (0, 0)                                             # n == 0: total 0
    assert eng.stat_rows(0, None, 0, None, None)[0] == b""
    assert int(eng.lib.wga_stat_rows_work_bytes(0)) == 8 * (0 + 0 // 1024 + 4)    # the documented formula
    assert int(eng.lib.wga_stat_rows_work_bytes(5000)) == 8 * (5000 + 5000 // 1024 + 4)
    # wga_f32_text: n == 0 is valid whatever the pointers, a null array with n > 0 is not
    lib, one = eng.lib, eng.upload(np.zeros(16, dtype=np.uint8))
    assert lib.wga_f32_text(eng.ctx, 0, None, None, None) == 0
    for k in range(3):
        p = [one.ptr, one.ptr, one.ptr]
        p[k] = None
        assert lib.wga_f32_text(eng.ctx, 1, *p) == E_INVALID_ARG, k
    # a second fill gives the same bytes; a workspace that another batch used before
    x = Raw(eng, a)
    x.count(len(want))
    assert x.fill() == want and x.fill() == want
    b = Arrays(eng, some(2, 1))
    y = Raw(eng, b, work=x.work)
    y.count(400)
    assert y.fill(3) == b"".join(want_rows(b.recs))


def item_stream(eng):
    """600 rows, three blocks of the fill (the smallest count with a block wholly in front of an altered total and one behind
    it), behind their count call; the scan of the row sizes is the caller's d_row_off"""
    recs = some(600, 3)
    a = Arrays(eng, recs)
    x = Raw(eng, a)
    want = b"".join(want_rows(recs))
    assert x.count(len(want)) == len(want)

    def fill(total_bytes, d_out):
        assert x.call(d_out, total=total_bytes) == total_bytes
    return ti.Stream(eng, x.row_off, 0, 600, want, fill)


def check_abi_fill_short_total(eng):
    ti.check_short_total(item_stream(eng))


def check_abi_fill_scan_one_off(eng):
    """a d_row_off altered between the calls: kCheckSize keeps the two rows around the altered entry unwritten"""
    ti.check_scan_one_off(item_stream(eng), size_checked=True)


def random_recs(seed):
    rnd = random.Random(7000 + seed)
    n = 40 + (seed * 67) % 700
    big = (0, 1, 9, 10, 99, 12345, 10 ** 6, (1 << 24) + 1, (1 << 32) - 1, 1 << 32, 10 ** 12, (1 << 53) + 1, 10 ** 19 - 1, U64)
    recs = []
    for _ in range(n):
        wild = rnd.random() < 0.1
        c = {f: (rnd.choice(big) if wild else rnd.randrange(10 ** rnd.randrange(1, 8))) for f in ref.COUNT_FIELDS}
        if rnd.random() < 0.7:
            c["inv_ev"] = 0
        name = b"ref.chr%d" % rnd.randrange(25) if rnd.random() < 0.95 else b'odd"\t%d' % rnd.randrange(9)
        recs.append(rec(rname=name, qname=b"qry.ctg%d" % rnd.randrange(40), ref_size=rnd.randrange(1, 4 * 10 ** 9),
                        ref_start=rnd.randrange(10 ** 9), query_size=rnd.choice(big), query_start=rnd.randrange(10 ** 9), c=c))
    return recs


def check_abi_random(eng, seeds):
    for seed in seeds:
        check(eng, random_recs(seed), shift=seed % 16)


# ---- the command -------------------------------------------------------------------------------------------------------------------
def three_ways(cli, *args, want=None, env=None, to=None, gz=False):
    """the command under the device writer and under WGA_STAT_WRITER=host: the same bytes (of stdout, or of the file `to` that -o
    names), exit status and message; under WGA_TIMING=1 a run that writes rows names the writer that ran, and one without -e
    names neither; and, where `want` is given, the restatement's bytes"""
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
    if dev[0] == 0 and "-e" in args and dev[1]:                                   # an input without a record has no piece
        assert "stat rows (device)" in dev[3] and "stat rows (host)" not in dev[3], dev[3]
        assert "stat rows (host)" in host[3] and "stat rows (device)" not in host[3], host[3]
    elif "-e" not in args:
        assert "stat rows (" not in dev[3] + host[3]
    if want is not None:
        assert dev[1] == want, (args, first_difference(dev[1], want))
    return dev[:3]


def random_cigar(rnd, mean=8):
    return "".join("%d%s" % (rnd.choice((1, 1, 2, 9, 10, 33, 120)), rnd.choice("M=XIDM")) for _ in range(rnd.randrange(1, 2 * mean)))


def paf_case(seed, n, targets=(b"c 1", b"c1", b"c10", b"c2", b"c 1"), queries=(b"q1", b"qry.2", b"q")):
    """n PAF records with the targets interleaved: (the file's text, the restatement's records)"""
    rnd = random.Random(8100 + seed)
    lines, records = [], []
    for k in range(n):
        cg = random_cigar(rnd)
        neg = rnd.random() < 0.5
        c = orc.parse_paf_to_cigar("cg:Z:" + cg, neg)
        t, q = targets[k % len(targets)], queries[(k // 2) % len(queries)]
        tl, ts, ql, qs = 10 ** 8 + k, rnd.randrange(10 ** 7), 10 ** 7 + 3 * k, rnd.randrange(10 ** 6)
        lines.append(b"%s\t%d\t%d\t%d\t%s\t%s\t%d\t%d\t%d\t%d\t%d\t60\tcg:Z:%s\n" % (
            q, ql, qs, qs + 50, b"-" if neg else b"+", t, tl, ts, ts + 50, c[0], c[0] + c[1], cg.encode()))
        records.append((t, tl, ts, q, ql, qs, c))
    return b"".join(lines), records


def check_cli_paf(cli, tmp_path):
    text, records = paf_case(1, 90)
    paf = write(tmp_path, "a.paf", text)
    want = ref.table(records)
    first = [ln.split(b"\t")[0] for ln in want.split(b"\n")[1:-1]]
    assert first == [b"c 1", b"c1", b"c 1"] * 18 + [b"c2"] * 18 + [b"c10"] * 18    # "c 1" and "c1": one rank, in input order
    assert three_ways(cli, "stat", "-f", "paf", "-e", paf, want=want) == (0, want, "")
    # several pieces, the targets interleaved across them
    chunk = len(text) // 4
    assert three_ways(cli, "stat", "-f", "paf", "-e", paf, want=want, env={"WGA_CHUNK_BYTES": str(chunk)}) == (0, want, "")
    # into a .gz file
    assert three_ways(cli, "stat", "-f", "paf", "-e", paf, want=want, to=str(tmp_path / "x.tsv.gz"), gz=True) == (0, want, "")
    assert len(text) // chunk >= 3
    # without -e nothing changes: one output under both settings, no label
    rc, merged, msg = three_ways(cli, "stat", "-f", "paf", paf)
    assert rc == 0 and msg == "" and merged.count(b"\n") == 1 + len({(r[0], r[1], r[3], r[4]) for r in records})


def check_cli_paf_host_reader(cli, tmp_path):
    """WGA_PAF_READER=host and a quoted name: the csv reader takes the quotes off, the writer puts them back on"""
    text, records = paf_case(2, 40, targets=(b"chr1", b"t\tab", b'q"uote'))
    text = text.replace(b'\tq"uote\t', b'\t"q""uote"\t').replace(b"\tt\tab\t", b'\t"t\tab"\t')
    paf = write(tmp_path, "q.paf", text)
    want = ref.table(records)
    assert b'"q""uote"\t' in want and b'"t\tab"\t' in want
    assert three_ways(cli, "stat", "-f", "paf", "-e", paf, want=want) == (0, want, "")          # a quote: the host reader's anyway
    plain, records = paf_case(3, 40)
    paf = write(tmp_path, "h.paf", plain)
    assert three_ways(cli, "stat", "-f", "paf", "-e", paf, want=ref.table(records), env={"WGA_PAF_READER": "host"})[0] == 0


def check_cli_empty_and_errors(cli, tmp_path):
    empty = write(tmp_path, "e.paf", b"")
    assert three_ways(cli, "stat", "-f", "paf", "-e", empty, want=b"") == (0, b"", "")
    assert three_ways(cli, "stat", "-e", write(tmp_path, "e.maf", b"##maf version=1\n\n"), want=b"") == (0, b"", "")
    # a bad CIGAR in the last piece: nothing is written, the same message and exit status
    text, _ = paf_case(4, 60)
    lines = text.split(b"\n")[:-1]
    lines[-3] += b"3N"
    bad = write(tmp_path, "b.paf", b"\n".join(lines) + b"\n")
    to = write(tmp_path, "b.tsv", b"")
    assert three_ways(cli, "stat", "-f", "paf", "-e", bad, env={"WGA_CHUNK_BYTES": str(len(text) // 4)}) == (1, b"", "CIGAR OP `N` invalid")
    assert three_ways(cli, "stat", "-f", "paf", "-e", bad, to=to) == (1, b"", "CIGAR OP `N` invalid")
    lines[-3] = lines[-3][:-2] + b"7"                                             # a number without an op: the tokeniser's error
    rc, out, msg = three_ways(cli, "stat", "-f", "paf", "-e", write(tmp_path, "t.paf", b"\n".join(lines) + b"\n"))
    assert rc == 1 and out == b"" and msg != ""


BASES = b"ACGTacgtNn"


def maf_case(seed, n, targets=(b"c9", b"c1", b"c10", b"c2", b"c1"), third=True):
    """n MAF blocks of a target, a query and (third) a second query: (the file's text, the restatement's records for the first
    query, ... for the second)"""
    rnd = random.Random(8700 + seed)
    out, recs1, recs2 = [b"##maf version=1 scoring=none\n\n"], [], []

    def rows(cols):
        t, q = bytearray(), bytearray()
        for _ in range(cols):
            x = rnd.random()
            t.append(45 if x < 0.08 else BASES[rnd.randrange(10)])
            q.append(45 if 0.08 <= x < 0.16 else (t[-1] if x < 0.8 and t[-1] != 45 else BASES[rnd.randrange(10)]))
        return bytes(t), bytes(q)

    for k in range(n):
        cols = rnd.choice((1, 7, 60, 200, 333))
        t, q = rows(cols)
        _, q2 = rows(cols)
        tn = targets[k % len(targets)]
        tsize, tstart, tali = 10 ** 8 + k, rnd.randrange(10 ** 7), cols - t.count(b"-")
        out.append(b"a score=%d\ns %s %d %d + %d %s\n" % (k, tn, tstart, tali, tsize, t))
        for name, row, into in ((b"qA.%d" % (k % 3), q, recs1), (b"qB", q2, recs2))[:2 if third else 1]:
            neg = rnd.random() < 0.5
            qsize, qstart, qali = 10 ** 7 + k, rnd.randrange(10 ** 6), cols - row.count(b"-")
            out.append(b"s %s %d %d %s %d %s\n" % (name, qstart, qali, b"-" if neg else b"+", qsize, row))
            c, _ = orc.parse_maf_seq_to_cigar(t, row, neg)
            into.append((tn, tsize, tstart, name, qsize, qsize - qstart - qali if neg else qstart, c))
        out.append(b"\n")
    return b"".join(out), recs1, recs2


def check_cli_maf(cli, tmp_path):
    text, recs1, recs2 = maf_case(1, 70)
    maf = write(tmp_path, "a.maf", text)
    want1, want2 = ref.table(recs1), ref.table(recs2)
    assert three_ways(cli, "stat", "-e", maf, want=want1) == (0, want1, "")
    assert three_ways(cli, "stat", "-e", "-q", "qB", maf, want=want2) == (0, want2, "")       # the named query of a multi-query file
    # several pieces (into a .gz file), and the host reader with the named query
    env = {"WGA_CHUNK_BYTES": str(len(text) // 4)}
    assert three_ways(cli, "stat", "-e", maf, want=want1, env=env, to=str(tmp_path / "m.tsv.gz"), gz=True) == (0, want1, "")
    assert three_ways(cli, "stat", "-e", "-q", "qB", maf, want=want2, env={"WGA_MAF_READER": "host"}) == (0, want2, "")
    assert three_ways(cli, "stat", maf)[0] == 0                                               # without -e: no label, one output


def check_cli_gpus(cli, tmp_path, gpus=2):
    """--gpus N: the counters meet on the host and device 0 writes the rows — the bytes of one device, also for a failing file"""
    text, records = paf_case(5, 60)
    paf = write(tmp_path, "g.paf", text)
    want = ref.table(records)
    g = ("--gpus", str(gpus))
    for env in ({"WGA_CHUNK_BYTES": str(len(text) // 3)}, {"WGA_PAF_READER": "host"}):
        assert three_ways(cli, *g, "stat", "-f", "paf", "-e", paf, want=want, env=env) == (0, want, ""), env
    lines = text.split(b"\n")[:-1]
    lines[50] += b"3N"
    bad = write(tmp_path, "gb.paf", b"\n".join(lines) + b"\n")
    assert three_ways(cli, *g, "stat", "-f", "paf", "-e", bad) == (1, b"", "CIGAR OP `N` invalid")
    mtext, recs1, recs2 = maf_case(2, 40)
    maf = write(tmp_path, "g.maf", mtext)
    assert three_ways(cli, *g, "stat", "-e", maf, want=ref.table(recs1), env={"WGA_CHUNK_BYTES": str(len(mtext) // 3)})[0] == 0
    assert three_ways(cli, *g, "stat", "-e", "-q", "qB", maf, want=ref.table(recs2), env={"WGA_MAF_READER": "host"})[0] == 0
