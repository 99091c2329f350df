"""The csv rows of `dotplot -m overview` on the device (K34): the C-ABI entries (Engine.dotplot_overview, Engine.f64_text) against
dotplot_overview_ref (the restatement from dotplot.rs, numpy.float64 and Dragon4), and the command with its device writer against
WGA_DOTPLOT_WRITER=host and the restatement over the oracle's counters.
Imported by test_emu_dotplot_overview.py (emulator build, CPU) and test_gpu_dotplot_overview.py (the product on a GPU); each
provides the `cli` and `eng` fixtures."""
import ctypes as C
import functools
import random

import numpy as np

import dotplot_overview_ref as ref
import maf2paf_cases as m2p
import oracle_py as orc
import text_items_cases as ti
from chain_split_cases import write
from wgatools_amd.engine import COUNTS_DTYPE, DOTPLOT_OV_HEAD_DTYPE

U64 = (1 << 64) - 1
E_INVALID_ARG = -1
COUNTS = (0, 1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2049)            # the wave, block and scan-partial borders
WIDTHS = (0, 1 << 32, 10 ** 19 - 1, U64)                                       # 1, 10, 19 and 20 digits
STAGE = 256 * 112                                                              # WGA_DOTPLOT_OV_STAGE
HOST_WRITER = {"WGA_DOTPLOT_WRITER": "host"}
DEVICE_PHASE, HOST_PHASE = "dotplot rows (device)", "dotplot rows (host)"


# ---- records and arrays ----------------------------------------------------------------------------------------------------------
def rec(rname=b"tchr", qname=b"qchr", ref_start=100, ref_end=600, q_first=700, q_second=1200, match=450, align_size=500):
    return dict(rname=rname, qname=qname, ref_start=ref_start, ref_end=ref_end, q_first=q_first, q_second=q_second, match=match,
                align_size=align_size)


def some(n, k0=0):
    """n records with names and numbers of several widths and the identity in several layouts"""
    out = []
    for k in range(k0, k0 + n):
        a = 10 ** (k % 9) + 3 * k
        out.append(rec(rname=b"t" * (1 + k % 5), qname=b"q%d" % (k % 11), ref_start=10 ** (k % 7), ref_end=10 ** (k % 7) + a,
                       q_first=7 * k, q_second=7 * k + a + k % 3, match=a - (a * (k % 13)) // 17, align_size=a))
    return out


def want_rows(recs, no_identity=False):
    return [ref.row(r["ref_start"], r["ref_end"], r["q_first"], r["q_second"], r["rname"], r["qname"], r["match"], r["align_size"],
                    no_identity) for r in recs]


class Arrays:
    """wga_dotplot_overview's arrays for a list of records: the names back to back in one buffer (16 bytes of slack behind), one
    head and one set of counters per record.  A record's `spans` = ((rname_off, rname_len), (qname_off, qname_len)) replaces its
    own."""

    def __init__(self, eng, recs):
        self.eng, self.recs, self.n = eng, recs, len(recs)
        names = bytearray()
        heads = np.zeros(self.n + 1, dtype=DOTPLOT_OV_HEAD_DTYPE)
        cnt = np.zeros(self.n + 1, dtype=COUNTS_DTYPE)
        for k, r in enumerate(recs):
            h = heads[k]
            for f in ("ref_start", "ref_end", "q_first", "q_second", "align_size"):
                h[f] = r[f]
            h["rname_off"], h["rname_len"] = len(names), len(r["rname"])
            names += r["rname"]
            h["qname_off"], h["qname_len"] = len(names), len(r["qname"])
            names += r["qname"]
            cnt[k]["match"] = r["match"]
            for f in COUNTS_DTYPE.names:                                          # no other counter is read
                if f != "match":
                    cnt[k][f] = 0x7777777777777777
        self.names = bytes(names)
        for k, r in enumerate(recs):
            if "spans" in r:
                (heads[k]["rname_off"], heads[k]["rname_len"]), (heads[k]["qname_off"], heads[k]["qname_len"]) = r["spans"]
        self.heads, self.counts = heads, cnt
        self.d_names = eng.upload(np.frombuffer(self.names + b"\0" * 16, dtype=np.uint8))
        self.d_heads, self.d_counts = eng.upload(heads), eng.upload(cnt)

    def args(self, no_identity=False):
        return self.n, self.d_names, len(self.names), self.d_heads, None if no_identity else self.d_counts, no_identity


def first_difference(got, exp):
    k = next((i for i, (x, y) in enumerate(zip(got, exp)) if x != y), min(len(got), len(exp)))
    return len(got), len(exp), k, got[max(0, k - 60):k + 60], exp[max(0, k - 60):k + 60]


def check(eng, recs, want=None, shift=0, no_identity=False):
    """both calls (Engine.dotplot_overview checks the guards around the text and that the total stays): the text is the
    restatement's rows in input order, and row_off their prefix sums"""
    a = Arrays(eng, recs)
    rows = want if want is not None else want_rows(recs, no_identity)
    text, row_off = eng.dotplot_overview(*a.args(no_identity), out_shift=shift)
    exp = b"".join(rows)
    assert text == exp, (len(recs), shift, first_difference(text, exp))
    assert [int(v) for v in row_off] == list(np.cumsum([0] + [len(r) for r in rows])), (len(recs), shift)
    return text


# ---- the C-ABI entry ---------------------------------------------------------------------------------------------------------------
def check_abi_record_counts(eng, ns=COUNTS):
    for n in ns:
        check(eng, some(n, n % 7))
        check(eng, some(n, n % 5), no_identity=True)                              # d_counts == NULL


class Raw:
    """the two calls by hand with guards around everything a call writes: 8 words behind row_off's n + 1, 64 bytes around d_out"""
    GUARD = 64

    def __init__(self, eng, a, work=None, no_identity=False):
        self.eng, self.a, self.no_identity = eng, a, no_identity
        self.work = work if work is not None else eng.empty(max(int(eng.lib.wga_dotplot_overview_work_bytes(a.n)), 16), np.uint8)
        self.row_off = eng.upload(np.full(a.n + 1 + 8, 0xA5A5A5A5A5A5A5A5, dtype=np.uint64))
        self.total = None

    def call(self, out_ptr, total=None):
        n, names, nb, heads, cnt, noid = self.a.args(self.no_identity)
        tot = C.c_uint64(total if total is not None else self.total if self.total is not None else 7)
        rc = self.eng.lib.wga_dotplot_overview(self.eng.ctx, n, names.ptr, nb, heads.ptr, cnt.ptr if cnt is not None else None,
                                               1 if noid else 0, self.work.ptr, self.row_off.ptr, C.byref(tot), out_ptr)
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
    call and after the fill, and so do the 8 words behind d_row_off; the same arguments for both calls"""
    for n in (1, 3, 257):
        recs = some(n, 2)
        a = Arrays(eng, recs)
        rows = want_rows(recs)
        exp = b"".join(rows)
        for shift in range(16):
            x = Raw(eng, a, no_identity=shift == 7)
            want = exp if shift != 7 else b"".join(want_rows(recs, True))
            assert x.count(len(want)) == len(want)
            if shift != 7:
                assert [int(v) for v in x.row_off.numpy()[:n + 1]] == list(np.cumsum([0] + [len(r) for r in rows]))
            assert x.fill(shift) == want, (n, shift)


def check_abi_numbers(eng):
    """every integer column at 1, 10, 19 and 20 digits; match and align_size at those widths too"""
    recs = []
    for k, w in enumerate(WIDTHS):
        v = WIDTHS[k:] + WIDTHS[:k]
        recs.append(rec(ref_start=v[0], ref_end=v[1], q_first=v[2], q_second=v[3], match=v[1], align_size=v[2]))
        recs.append(rec(ref_start=w, ref_end=w, q_first=w, q_second=w, match=w, align_size=w))
    text = check(eng, recs)
    assert b",18446744073709551615," in text and b",9999999999999999999," in text and b",4294967296," in text
    assert text.startswith(b"0,4294967296,9999999999999999999,18446744073709551615,")
    cols = [ln.split(b",") for ln in text.split(b"\n")[:-1]]
    for c in range(4):
        assert {len(r[c]) for r in cols} == {1, 10, 19, 20}, c
    check(eng, recs, no_identity=True)


def check_abi_identity(eng):
    """the identity column through the counter and the divisor"""
    cases = [
        ((0, 0), b"NaN"), ((8, 0), b"inf"), ((U64, 0), b"inf"),                  # align_size == 0
        ((0, 7), b"0.0"), ((77, 77), b"1.0"), ((1, 3), b"0.3333333333333333"), ((2, 3), b"0.6666666666666666"),
        ((1, 10), b"0.1"), ((3, 10), b"0.3"), ((9, 8), b"1.125"),                # match > align_size
        ((10 ** 6, 1), b"1000000.0"), ((10 ** 15, 1), b"1000000000000000.0"),    # kk = 16: still plain
        ((10 ** 16, 1), b"1e16"), ((10 ** 16 + 2, 1), b"1.0000000000000002e16"),
        ((1, 10 ** 4), b"0.0001"), ((1, 10 ** 5), b"0.00001"), ((1, 10 ** 6), b"1e-6"), ((3, 2 * 10 ** 6), b"1.5e-6"),
        (((1 << 53) + 1, 1), b"9007199254740992.0"),                              # 2^53 + 1 -> 2^53: a tie, to even
        (((1 << 53) + 3, 1), b"9007199254740996.0"),                              # ... and up to 2^53 + 4
        ((U64, 1), b"1.8446744073709552e19"), ((1, U64), b"5.421010862427522e-20"), ((U64, U64), b"1.0"),
        ((U64 - 1, U64), b"1.0"), ((1 << 63, 3), None), ((12345678901234567, 10 ** 17), None), ((450, 500), b"0.9"),
    ]
    recs = [rec(match=m, align_size=a) for (m, a), _ in cases]
    rows = want_rows(recs)
    for row, (ma, exp) in zip(rows, cases):
        assert exp is None or row.split(b",")[4] == exp, (ma, row)
    text = check(eng, recs, rows)
    assert text.startswith(b"100,600,700,1200,NaN,tchr,qchr\n100,600,700,1200,inf,tchr,qchr\n")
    text = check(eng, recs, no_identity=True)
    assert text == b"100,600,700,1200,1.0,tchr,qchr\n" * len(recs)


def check_abi_names(eng):
    long300, long5k = bytes(65 + k % 26 for k in range(300)), bytes(97 + k % 26 for k in range(5000))
    recs = [rec(rname=b"", qname=b""), rec(rname=b"a", qname=b"b"), rec(rname=long300, qname=long300[::-1]),
            rec(rname=b"t,1", qname=b'q"uote"'), rec(rname=b"c\rr", qname=b"l\nf"), rec(rname=b'"', qname=b'"",""'),
            rec(rname=b"plain name", qname=b"tab\tsemi;")]
    rows = want_rows(recs)
    assert rows[0].endswith(b",,\n") and rows[3].endswith(b',"t,1","q""uote"""\n') and rows[4].endswith(b',"c\rr","l\nf"\n')
    assert rows[5].endswith(b',"""",""""","""""\n') and rows[6].endswith(b",plain name,tab\tsemi;\n")
    check(eng, recs, rows)
    check(eng, recs, no_identity=True)
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
    # names of 5 000 bytes: seven of them make a block's stretch longer than the stage and it is written directly, the blocks
    # around it staged; one alone is still staged
    for at in ((0,), (255,), (256,), (300,), tuple(range(100, 107)), tuple(range(250, 262))):
        recs = some(600, 1)
        for k in at:
            recs[k] = rec(rname=long5k, qname=b"q", match=3)
        text = check(eng, recs)
        assert (len(at) * 5000 > STAGE) == (len(at) > 1) and len(text) > 5000 * len(at)
    recs = some(40)
    recs[7] = rec(rname=b"r", qname=b'x"' + long5k * 6 + b",")
    check(eng, recs, shift=5)


LAYOUT = (1e-5, np.nextafter(1e-5, 0), 1e16, np.nextafter(1e16, 0), 1e15, 1e-4, 123456.789)
NAMED = (5e-324, 2.2250738585072014e-308, np.nextafter(2.2250738585072014e-308, 0), 1.7976931348623157e308, 2.0 ** 53, 1e23,
         9.5367431640625e-7, 0.3, 1.0 / 3.0, 2.0 / 3.0)
SPECIAL_BITS = (0x0000000000000000, 0x8000000000000000, 0x7FF0000000000000, 0xFFF0000000000000, 0x7FF8000000000000,
                0x7FF0000000000001, 0xFFFFFFFFFFFFFFFF)


def bits_of(values):
    return np.array(values, dtype=np.float64).view(np.uint64)


@functools.lru_cache(maxsize=None)
def f64_patterns():
    """(the patterns, the restatement's texts): the specials, the layout borders and the named values with their negatives, every
    power of two, every a / b with 0 <= a, b <= 64, every exponent field with the mantissas 0, 1, 2^51 and 2^52 - 1, 50 000
    patterns and 50 000 ratios of 1 .. 64-bit numbers from fixed seeds.  Computed once and shared."""
    parts = [np.array(SPECIAL_BITS, dtype=np.uint64), bits_of(LAYOUT), bits_of(NAMED), bits_of(LAYOUT) | np.uint64(1 << 63),
             bits_of(NAMED) | np.uint64(1 << 63)]
    pow2 = [k << 52 for k in range(1, 2047)] + [1 << k for k in range(52)]        # 2^-1022 .. 2^1023, 2^-1074 .. 2^-1023
    assert len(pow2) == 1023 + 1074 + 1
    parts.append(np.array(pow2, dtype=np.uint64))
    with np.errstate(divide="ignore", invalid="ignore"):
        a = np.arange(65, dtype=np.uint64).astype(np.float64)
        parts.append((a[:, None] / a[None, :]).reshape(-1).view(np.uint64))
        e = np.arange(2048, dtype=np.uint64) << np.uint64(52)
        parts.append((e[:, None] | np.array([0, 1, 1 << 51, (1 << 52) - 1], dtype=np.uint64)[None, :]).reshape(-1))
        rnd = np.random.RandomState(20261021)
        parts.append(rnd.randint(0, 1 << 32, size=50000, dtype=np.uint64) << np.uint64(32) | rnd.randint(0, 1 << 32, size=50000, dtype=np.uint64))
        wide = lambda: (rnd.randint(0, 1 << 32, size=50000, dtype=np.uint64) << np.uint64(32) | rnd.randint(0, 1 << 32, size=50000, dtype=np.uint64))
        num = (wide() >> rnd.randint(0, 64, size=50000).astype(np.uint64))         # 1 .. 64 bits
        den = (wide() >> rnd.randint(0, 64, size=50000).astype(np.uint64))
        parts.append((num.astype(np.float64) / den.astype(np.float64)).view(np.uint64))
    bits = np.concatenate(parts)
    return bits, ref.f64_texts(bits)


def check_ref_layouts():
    """the restatement prints the named values as ryu does (the pretty::format64 cases, by hand)"""
    t = ref.f64_text
    assert [ref.f64_text_of_bits(b) for b in SPECIAL_BITS] == [b"0.0", b"-0.0", b"inf", b"-inf", b"NaN", b"NaN", b"NaN"]
    assert [t(v) for v in LAYOUT] == [b"0.00001", b"9.999999999999999e-6", b"1e16", b"9999999999999998.0", b"1000000000000000.0",
                                      b"0.0001", b"123456.789"]
    assert [t(v) for v in NAMED] == [b"5e-324", b"2.2250738585072014e-308", b"2.225073858507201e-308", b"1.7976931348623157e308",
                                     b"9007199254740992.0", b"1e23", b"9.5367431640625e-7", b"0.3", b"0.3333333333333333",
                                     b"0.6666666666666666"]
    assert t(-123456.789) == b"-123456.789" and t(-1e-20) == b"-1e-20" and t(-1.5e300) == b"-1.5e300"
    assert t(2.0 ** -1074) == b"5e-324" and t(2.0 ** 1023) == b"8.98846567431158e307" and t(2.0 ** -1022) == b"2.2250738585072014e-308"
    assert max(len(t(v)) for v in (-1.2345678901234567e-308, -2.2250738585072014e-308)) == 24


def check_f64_text(eng):
    bits, want = f64_patterns()
    got = eng.f64_text(bits)
    bad = [(hex(int(b)), g, w) for b, g, w in zip(bits, got, want) if g != w]
    assert not bad, (len(bad), bad[:10])
    assert eng.f64_text(np.zeros(0, dtype=np.uint64)) == []


def raw(eng, a, n=None, work=True, null=(), names_bytes=None, total=True, no_identity=False):
    d_work = eng.empty(max(int(eng.lib.wga_dotplot_overview_work_bytes(a.n)), 16), np.uint8)
    row_off = eng.empty(a.n + 2, np.uint64)
    tot = C.c_uint64(7)
    p = dict(names=a.d_names.ptr, heads=a.d_heads.ptr, counts=a.d_counts.ptr, row_off=row_off.ptr)
    for k in null:
        p[k] = None
    rc = eng.lib.wga_dotplot_overview(eng.ctx, a.n if n is None else n, p["names"], len(a.names) if names_bytes is None else names_bytes,
                                      p["heads"], p["counts"], 1 if no_identity else 0, d_work.ptr if work else None, p["row_off"],
                                      C.byref(tot) if total else None, None)
    return rc, tot.value


def check_abi_arguments(eng):
    recs = some(3)
    a = Arrays(eng, recs)
    want, want_1 = b"".join(want_rows(recs)), b"".join(want_rows(recs, True))
    assert raw(eng, a) == (0, len(want))
    for n in (None, 0):                                                           # whatever the count
        assert raw(eng, a, work=False, n=n)[0] == E_INVALID_ARG and raw(eng, a, total=False, n=n)[0] == E_INVALID_ARG
    for null in ("names", "heads", "counts", "row_off"):
        assert raw(eng, a, null=(null,))[0] == E_INVALID_ARG, null
        assert raw(eng, a, n=0, null=(null,)) == (0, 0), null
    assert raw(eng, a, null=("counts",), no_identity=True) == (0, len(want_1))    # d_counts only when !no_identity
    for null in ("names", "heads", "row_off"):
        assert raw(eng, a, null=(null,), no_identity=True)[0] == E_INVALID_ARG, null
    assert raw(eng, a, null=("names",), names_bytes=0) == (0, len(b"".join(want_rows([dict(r, rname=b"", qname=b"") for r in recs]))))
    assert raw(eng, a, n=0xFFFFFFF1)[0] == E_INVALID_ARG and raw(eng, a, n=0xFFFFFFFF, no_identity=True)[0] == E_INVALID_ARG
    assert raw(eng, a, n=0) == (0, 0)                                             # n == 0: total 0
    assert eng.dotplot_overview(0, None, 0, None, None)[0] == b""
    assert int(eng.lib.wga_dotplot_overview_work_bytes(0)) == 8 * (0 + 0 // 1024 + 4)    # the documented formula
    assert int(eng.lib.wga_dotplot_overview_work_bytes(5000)) == 8 * (5000 + 5000 // 1024 + 4)
    # wga_f64_text: n == 0 is valid whatever the pointers, a null array with n > 0 is not
    lib, one = eng.lib, eng.upload(np.zeros(32, dtype=np.uint8))
    assert lib.wga_f64_text(eng.ctx, 0, None, None, None) == 0
    for k in range(3):
        p = [one.ptr, one.ptr, one.ptr]
        p[k] = None
        assert lib.wga_f64_text(eng.ctx, 1, *p) == E_INVALID_ARG, k
    assert lib.wga_f64_text(eng.ctx, 0xFFFFFFF1, one.ptr, one.ptr, one.ptr) == E_INVALID_ARG
    # a second fill gives the same bytes; a workspace that another batch used before
    x = Raw(eng, a)
    x.count(len(want))
    assert x.fill() == want and x.fill() == want
    b = Arrays(eng, some(2, 1))
    y = Raw(eng, b, work=x.work)
    y.count(400)
    assert y.fill(3) == b"".join(want_rows(b.recs))


def item_stream(eng):
    """600 rows, three blocks of the fill, behind their count call; the scan of the row sizes is the caller's d_row_off"""
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
    rnd = random.Random(7400 + seed)
    n = 40 + (seed * 67) % 700
    big = (0, 1, 9, 10, 99, 12345, 10 ** 6, (1 << 24) + 1, (1 << 32) - 1, 1 << 32, 10 ** 12, (1 << 53) + 1, 10 ** 19 - 1, U64)
    recs = []
    for _ in range(n):
        wild = rnd.random() < 0.1
        num = lambda: rnd.choice(big) if wild else rnd.randrange(10 ** rnd.randrange(1, 10))
        name = b"ref.chr%d" % rnd.randrange(25) if rnd.random() < 0.95 else b'odd",%d' % rnd.randrange(9)
        recs.append(rec(rname=name, qname=b"qry.ctg%d" % rnd.randrange(40), ref_start=num(), ref_end=num(), q_first=num(), q_second=num(),
                        match=num(), align_size=num()))
    return recs


def check_abi_random(eng, seeds):
    for seed in seeds:
        check(eng, random_recs(seed), shift=seed % 16, no_identity=seed % 4 == 3)


# ---- the command -------------------------------------------------------------------------------------------------------------------
def three_ways(cli, *args, want=None, env=None, host_rows=False):
    """the command under the device writer and under WGA_DOTPLOT_WRITER=host: the same bytes, exit status and message; under
    WGA_TIMING=1 each run names the writer that ran (host_rows: the rows are the host's under both, a MAF with -d); and, where
    `want` is given, the restatement's bytes"""
    env = env or {}
    dev, host = (m2p.timed(cli, list(args), e) for e in (env, dict(env, **HOST_WRITER)))
    assert dev[0] in (0, 1) and dev[:3] == host[:3], (args, dev[0], host[0], dev[2], host[2], first_difference(dev[1], host[1]))
    if dev[0] == 0:
        if host_rows:
            assert HOST_PHASE in dev[3] and DEVICE_PHASE not in dev[3], dev[3]
        else:
            assert DEVICE_PHASE in dev[3] and HOST_PHASE not in dev[3], dev[3]
        assert HOST_PHASE in host[3] and DEVICE_PHASE not in host[3], host[3]
    if want is not None:
        assert dev[1] == want, (args, first_difference(dev[1], want))
    return dev[:3]


OVERVIEW = ("dotplot", "-m", "overview", "--out-format", "csv")


def random_cigar(rnd, mean=8):
    return "".join("%d%s" % (rnd.choice((1, 1, 2, 9, 10, 33, 120)), rnd.choice("M=XIDM")) for _ in range(rnd.randrange(1, 2 * mean)))


def paf_case(seed, n, targets=(b"chr1", b"c,2", b"chr10", b"t"), queries=(b"q1", b"qry.2", b"q")):
    """n PAF records: (the file's text, the restatement's records over the oracle's counters).  The target span is that of the
    CIGAR, or 0 (identity NaN or inf), or 1 (identity above 1)"""
    rnd = random.Random(9100 + seed)
    lines, records = [], []
    for k in range(n):
        cg = random_cigar(rnd)
        neg = rnd.random() < 0.5
        c = orc.parse_paf_to_cigar("cg:Z:" + cg, neg)
        t, q = targets[k % len(targets)], queries[(k // 2) % len(queries)]
        ts, qs = rnd.randrange(10 ** 7), rnd.randrange(10 ** 6)
        te = ts + (c[0] + c[1] + c[5], 0, 1)[(k % 11 == 3) + (k % 11 == 7) * 2]
        qe = qs + c[0] + c[1] + c[3]
        lines.append(b"%s\t%d\t%d\t%d\t%s\t%s\t%d\t%d\t%d\t%d\t%d\t60\tcg:Z:%s\n" % (
            q, 10 ** 7 + 3 * k, qs, qe, b"-" if neg else b"+", t, 10 ** 8 + k, ts, te, c[0], c[0] + c[1], cg.encode()))
        records.append((t, ts, te, q, qs, qe, neg, c[0]))
    return b"".join(lines), records


def check_cli_paf(cli, tmp_path):
    """a PAF that the device reader takes: plain and -d, one piece and several"""
    text, records = paf_case(1, 90)
    paf = write(tmp_path, "a.paf", text)
    want, want_1 = ref.table(records), ref.table(records, True)
    assert b",NaN," in want or b",inf," in want
    assert b',"c,2",' in want
    assert three_ways(cli, *OVERVIEW, "-f", "paf", paf, want=want) == (0, want, "")
    assert three_ways(cli, *OVERVIEW, "-f", "paf", "-d", paf, want=want_1) == (0, want_1, "")
    env = {"WGA_CHUNK_BYTES": str(len(text) // 4)}
    assert three_ways(cli, *OVERVIEW, "-f", "paf", paf, want=want, env=env) == (0, want, "")
    assert three_ways(cli, *OVERVIEW, "-f", "paf", "-d", paf, want=want_1, env=env) == (0, want_1, "")
    # the pinned row of a record without a target span
    one = write(tmp_path, "nan.paf", b"q\t100\t0\t8\t+\tt\t100\t7\t7\t0\t0\t60\tcg:Z:8I\n")
    assert three_ways(cli, *OVERVIEW, "-f", "paf", one)[1] == ref.HEADER + b"7,7,0,8,NaN,t,q\n"


def check_cli_paf_host_reader(cli, tmp_path):
    """a quoted name makes the piece the host reader's: the csv reader takes the quotes off, the writer puts them back on; and
    WGA_PAF_READER=host on a plain file.  The names are then uploaded in a buffer of their own"""
    text, records = paf_case(2, 40, targets=(b"chr1", b"t,ab", b'q"uote'))
    text = text.replace(b'\tq"uote\t', b'\t"q""uote"\t')
    paf = write(tmp_path, "q.paf", text)
    want = ref.table(records)
    assert b',"q""uote",' in want and b',"t,ab",' in want
    assert three_ways(cli, *OVERVIEW, "-f", "paf", paf, want=want) == (0, want, "")
    assert three_ways(cli, *OVERVIEW, "-f", "paf", "-d", paf, want=ref.table(records, True))[0] == 0
    plain, records = paf_case(3, 40)
    paf = write(tmp_path, "h.paf", plain)
    assert three_ways(cli, *OVERVIEW, "-f", "paf", paf, want=ref.table(records), env={"WGA_PAF_READER": "host"})[0] == 0


def check_cli_empty_and_errors(cli, tmp_path):
    """no record: no header line; a record with a bad op leaves the output empty and gives the message of the host writer"""
    empty = write(tmp_path, "e.paf", b"")
    for d in ((), ("-d",)):
        rc, out, msg, _ = m2p.timed(cli, list(OVERVIEW) + ["-f", "paf", *d, empty], {})
        assert (rc, out, msg) == (0, b"", "")
        assert m2p.timed(cli, list(OVERVIEW) + [*d, write(tmp_path, "e.maf", b"##maf version=1\n\n")], {})[:3] == (0, b"", "")
    text, _ = paf_case(4, 60)
    lines = text.split(b"\n")[:-1]
    lines[-3] += b"3N"
    bad = write(tmp_path, "b.paf", b"\n".join(lines) + b"\n")
    assert three_ways(cli, *OVERVIEW, "-f", "paf", bad, env={"WGA_CHUNK_BYTES": str(len(text) // 4)}) == (1, b"", "CIGAR OP `N` invalid")
    assert three_ways(cli, *OVERVIEW, "-f", "paf", bad) == (1, b"", "CIGAR OP `N` invalid")
    assert three_ways(cli, *OVERVIEW, "-f", "paf", "-d", bad)[0] == 0             # -d: the ops are not read
    lines[-3] = lines[-3][:-2] + b"7"                                             # a number without an op: the tokeniser's error
    rc, out, msg = three_ways(cli, *OVERVIEW, "-f", "paf", write(tmp_path, "t.paf", b"\n".join(lines) + b"\n"))
    assert rc == 1 and out == b"" and msg != ""


BASES = b"ACGTacgtNn"


def maf_case(seed, n, targets=(b"c9", b"c1", b"c,10", b"c2", b"c1")):
    """n MAF blocks of a target, a query and a second query: (the file's text, the restatement's records for the first query,
    ... for the second)"""
    rnd = random.Random(9700 + seed)
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
        for name, row, into in ((b"qA.%d" % (k % 3), q, recs1), (b"qB", q2, recs2)):
            neg = rnd.random() < 0.5
            qsize, qstart, qali = 10 ** 7 + k, rnd.randrange(10 ** 6), cols - row.count(b"-")
            out.append(b"s %s %d %d %s %d %s\n" % (name, qstart, qali, b"-" if neg else b"+", qsize, row))
            c, _ = orc.parse_maf_seq_to_cigar(t, row, neg)
            q_lo = qsize - qstart - qali if neg else qstart
            into.append((tn, tstart, tstart + tali, name, q_lo, q_lo + qali, neg, c[0]))
        out.append(b"\n")
    return b"".join(out), recs1, recs2


def check_cli_maf(cli, tmp_path):
    text, recs1, recs2 = maf_case(1, 70)
    maf = write(tmp_path, "a.maf", text)
    want1, want2 = ref.table(recs1), ref.table(recs2)
    assert b',"c,10",' in want1
    assert three_ways(cli, *OVERVIEW, maf, want=want1) == (0, want1, "")
    assert three_ways(cli, *OVERVIEW, "-q", "qB", maf, want=want2) == (0, want2, "")     # the named query of a multi-query file
    # -d: no device holds anything of the blocks, the rows stay the host's
    want_1 = ref.table(recs1, True)
    assert three_ways(cli, *OVERVIEW, "-d", maf, want=want_1, host_rows=True) == (0, want_1, "")
    # several pieces, and the host reader with the named query (the names in a buffer of their own)
    env = {"WGA_CHUNK_BYTES": str(len(text) // 4)}
    assert three_ways(cli, *OVERVIEW, maf, want=want1, env=env) == (0, want1, "")
    assert three_ways(cli, *OVERVIEW, "-d", maf, want=want_1, env=env, host_rows=True) == (0, want_1, "")
    assert three_ways(cli, *OVERVIEW, "-q", "qB", maf, want=want2, env={"WGA_MAF_READER": "host"}) == (0, want2, "")


def check_cli_gpus(cli, tmp_path, gpus=2):
    """--gpus N: every device writes the rows of its contiguous range and the texts meet in input order — the bytes of one device,
    also for a failing file"""
    text, records = paf_case(5, 61)
    paf = write(tmp_path, "g.paf", text)
    want, want_1 = ref.table(records), ref.table(records, True)
    g = ("--gpus", str(gpus))
    for env in ({}, {"WGA_CHUNK_BYTES": str(len(text) // 3)}, {"WGA_PAF_READER": "host"}):
        assert three_ways(cli, *g, *OVERVIEW, "-f", "paf", paf, want=want, env=env) == (0, want, ""), env
        assert three_ways(cli, *g, *OVERVIEW, "-f", "paf", "-d", paf, want=want_1, env=env) == (0, want_1, ""), env
    lines = text.split(b"\n")[:-1]
    lines[50] += b"3N"
    bad = write(tmp_path, "gb.paf", b"\n".join(lines) + b"\n")
    assert three_ways(cli, *g, *OVERVIEW, "-f", "paf", bad) == (1, b"", "CIGAR OP `N` invalid")
    mtext, recs1, recs2 = maf_case(2, 41)
    maf = write(tmp_path, "g.maf", mtext)
    want1 = ref.table(recs1)
    assert three_ways(cli, *g, *OVERVIEW, maf, want=want1, env={"WGA_CHUNK_BYTES": str(len(mtext) // 3)}) == (0, want1, "")
    assert three_ways(cli, *g, *OVERVIEW, "-d", maf, want=ref.table(recs1, True), host_rows=True)[0] == 0
    assert three_ways(cli, *g, *OVERVIEW, "-q", "qB", maf, want=ref.table(recs2), env={"WGA_MAF_READER": "host"})[0] == 0
