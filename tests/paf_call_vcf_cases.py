"""K16 (`wga_paf_call_vcf`: the VCF rows of `call` on PAF) at kernel level, through the C-ABI only, against the oracle.
Imported by test_emu_paf_call_vcf.py (emulator build, CPU) and test_gpu_paf_call_vcf.py (the product on a GPU).

The expectation is never a restatement of the row layout: a clean record's text is orc.call_within_var_paf on the same
sequences; a record with an error ends in front of the first op whose CIGAR prefix the oracle refuses (its slice panic) or
prints with a REF / ALT character outside ACGTN (expect_record).  The text buffer is [guard + shift | text | guard]: the fill
pass must leave both guards as they were.

A record is the tuple (cigar text without the tag, strand is '-', t_name, q_name, t_start, t_end, q_start, q_end, fetched
target bytes, fetched query bytes)."""
import functools
import re

import numpy as np

import oracle_py as orc
from helpers import pack_records
from wgatools_amd.engine import OP_MAX_LEN, VCF_ERR_DTYPE, VCF_REC_DTYPE

NONE = 0xFFFFFFFFFFFFFFFF
GUARD_BYTE = 0xA5                     # no VCF row holds it: rows are 7-bit text
FILL = b"@"                           # between the pools' slices and the names: no base, so a read outside a slice shows
IUPAC = b"RYKMSWBDHVrykmU*"
HUGE = 10 ** 9                        # an `svlen` larger than every indel of the hand-built records
SVLENS = (0, 1, 2, 5, 50, HUGE)
TOKEN = re.compile(r"\d+[^\d]")
T_CONS, Q_CONS = "M=XDN", "M=XI"


# ---- records ---------------------------------------------------------------------------------------------------------------
def cigar_of(ops):
    return "".join("%d%s" % (ln, c) for c, ln in ops)


def mk(ops, neg=False, seed=0, t_name="chrT", q_name="qry.1", t_start=1000, q_start=2000, alpha=b"ACGT"):
    """a record from (op, length) pairs with random sequences as the command line fetches them: [start, end] inclusive"""
    rng = np.random.default_rng(seed)
    a = np.frombuffer(alpha, dtype=np.uint8)
    t_cons = sum(ln for c, ln in ops if c in T_CONS)
    q_cons = sum(ln for c, ln in ops if c in Q_CONS)
    t = a[rng.integers(0, len(a), t_cons + 1)].tobytes()
    q = a[rng.integers(0, len(a), q_cons + 1)].tobytes()
    return (cigar_of(ops), bool(neg), t_name, q_name, t_start, t_start + t_cons, q_start, q_start + q_cons, t, q)


def adv(ops, idx):
    """(target, query) bases in front of op `idx`"""
    return (sum(ln for c, ln in ops[:idx] if c in T_CONS), sum(ln for c, ln in ops[:idx] if c in Q_CONS))


def put(rec, row, pos, ch):
    """a copy of the record with byte `ch` at `pos` of its target ('t') or query ('q') sequence"""
    k = 8 if row == "t" else 9
    s = bytearray(rec[k])
    s[pos] = ch
    return rec[:k] + (bytes(s),) + rec[k + 1:]


def cut(rec, row, n):
    """a copy of the record whose target / query sequence is its first n bytes"""
    k = 8 if row == "t" else 9
    assert n < len(rec[k])
    return rec[:k] + (rec[k][:n],) + rec[k + 1:]


def with_neg(rec, neg):
    return rec[:1] + (bool(neg),) + rec[2:]


def snp_ops(n):
    """2 n ops: '=' of 3 and X of 1 in turn -> with `snp`, event e is op 2 e + 1"""
    return [("=", 3), ("X", 1)] * n


PATTERN = [("=", 3), ("X", 2), ("=", 4), ("I", 4), ("=", 3), ("D", 4), ("=", 2), ("X", 3)]   # op i is PATTERN[i % 8]


def pattern_ops(n):
    """with `snp` and svlen < 4: four events every eight ops (ops 1, 3, 5, 7); event e is op 2 e + 1"""
    return [PATTERN[i % 8] for i in range(n)]


# ---- the expectation -------------------------------------------------------------------------------------------------------
def _ref_alt(text):
    """the REF and ALT fields of all rows (a row has nine tabs, so the fields lie 9 apart), without <INV>"""
    f = text.split("\t")
    return [x for x in f[3::9] + f[4::9] if x != "<INV>"]


def dirty(text):
    return "".join(_ref_alt(text)).strip("ACGTN") != ""


def first_bad(text):
    """the first REF / ALT character outside ACGTN in the rows, REF before ALT; None"""
    for ln in text.splitlines():
        f = ln.split("\t")
        for field in (f[3], "" if f[4] == "<INV>" else f[4]):
            for ch in field:
                if ch not in "ACGTN":
                    return ch
    return None


def expect_record(rec, svlen, snp):
    """dict(text, kind, ch, op): the text the kernel owes and the error, from oracle calls on CIGAR prefixes.  op: the index
    of the failing op among the CIGAR's tokens, -1 for the <INV> row, None for a clean record.  The walk is monotone (a
    prefix that fails stays failing when ops are added), so the shortest failing prefix is found by bisection; to save oracle
    calls the search starts at the op that holds the sequences' first odd byte or their end (a guess that only decides
    where the search begins: the answer is the shortest prefix the oracle fails on, whatever the guess).  The prefix of no ops is
    the CIGAR `1=`: no row but the <INV> row of a '-' record, whose base is therefore checked first."""
    cg, neg, tn, qn, ts, te, qs, qe, t, q = rec
    ends = [m.end() for m in TOKEN.finditer(cg)]
    assert ends and ends[-1] == len(cg)

    @functools.lru_cache(maxsize=None)
    def run(p):
        try:
            return orc.call_within_var_paf(tn, qn, "cg:Z:" + (cg[:ends[p - 1]] if p else "1="), t, q, ts, te, qs, qe, neg, snp, svlen)
        except orc.OracleError as e:
            assert e.kind == 6, e       # ORC_PANIC: the reference's slice panic, no other error
            return None

    bad = lambda p: run(p) is None or dirty(run(p))
    n = len(ends)
    if not bad(n):
        return dict(text=run(n).encode(), kind=0, ch=None, op=None)
    if bad(0):
        return dict(text=b"", kind=1 if run(0) is None else 2, ch=None if run(0) is None else first_bad(run(0)), op=-1)
    lo, hi = 0, n                       # prefix lo is fine, prefix hi fails
    g = min(_guess(cg, "t", t), _guess(cg, "q", q), n - 1)
    if bad(g):
        hi = g
    else:
        lo, step = g, 1
        while lo + step < hi:
            if bad(lo + step):
                hi = lo + step
                break
            lo, step = lo + step, 2 * step
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if bad(mid):
            hi = mid
        else:
            lo = mid
    good = run(lo)
    if run(hi) is None:
        return dict(text=good.encode(), kind=1, ch=None, op=hi - 1)
    assert run(hi).startswith(good)
    return dict(text=good.encode(), kind=2, ch=first_bad(run(hi)[len(good):]), op=hi - 1)


_ODD = bytes(0 if x in b"ACGTNacgtn" else 1 for x in range(256))
_HEAL = bytes(x if x in b"ACGTNacgtn" else 78 for x in range(256))


def _guess(cg, row, seq):
    """the op in whose range the sequence's first byte outside ACGTNacgtn, or its end, lies"""
    at = seq.translate(_ODD).find(b"\1")
    cons = T_CONS if row == "t" else Q_CONS
    lens = np.cumsum([int(x[:-1]) if x[-1] in cons else 0 for x in TOKEN.findall(cg)])
    return int(np.searchsorted(lens, at if at >= 0 else len(seq), side="right"))


def healed_len(rec, svlen, snp, owed, clean=False):
    """bytes of the oracle's text of the record with every bad base replaced by a valid one and both sequences long enough:
    the most a fill pass that ignores the count pass's verdict could write.  Two kinds of record have no such text and count
    with what they owe: one with an indel no sequence has moved in front of (the oracle refuses it whatever the sequences),
    and one with a split indel (a row of 2^28 bases and more is not built here).  A clean record's is its own text."""
    cg, neg, tn, qn, ts, te, qs, qe, t, q = rec
    if clean:
        return owed
    toks = [(m.group()[-1], int(m.group()[:-1])) for m in TOKEN.finditer(cg)]
    if any(ln > OP_MAX_LEN for _, ln in toks):
        return owed
    heal = lambda s, n: s.translate(_HEAL) + b"A" * max(0, n - len(s))
    t2 = heal(t, max(len(t), sum(ln for c, ln in toks if c in T_CONS) + 1))
    q2 = heal(q, max(len(q), sum(ln for c, ln in toks if c in Q_CONS) + 1))
    try:
        return len(orc.call_within_var_paf(tn, qn, "cg:Z:" + cg, t2, q2, ts, te, qs, qe, neg, snp, svlen))
    except orc.OracleError:
        return owed


# ---- the driver ------------------------------------------------------------------------------------------------------------
def _pool(seqs):
    """the slices with filler between them, no offset a multiple of 16; a sequence that is the SAME object as the one in front
    of it shares its slice; an empty sequence lies inside the pool"""
    buf, offs, last = bytearray(FILL), [], None
    for s in seqs:
        if last is not None and s is last[0]:
            offs.append(last[1])
            continue
        while len(buf) % 16 == 0:
            buf += FILL
        offs.append(len(buf))
        last = (s, len(buf))
        buf += s + FILL * 3
    buf += FILL * 16
    return np.frombuffer(bytes(buf), dtype=np.uint8), offs


def run_k16_full(eng, recs, svlen, snp, guard, shift=0):
    """the C-ABI calls of `call` on PAF: K7 count, scan, K7 fill, K16 count (nbytes pre-filled with 0xFF, err with 0x5A), scan,
    K16 fill into [guard + shift | text | guard] pre-filled with 0xA5.
    -> (nbytes, err, out_off, the whole buffer, the event list, its offsets, each record's packed op count)"""
    n = len(recs)
    ops, op_off, errs = pack_records(eng, [r[0] for r in recs])
    assert not any(errs), errs
    batch = eng.make_batch(ops, op_off, np.array([r[1] for r in recs], dtype=np.uint8))
    cnt = eng.paf_call_events(batch, svlen, snp)
    ev_off = eng.exclusive_scan_u64(n, cnt)
    eo = ev_off.numpy()
    ev = eng.empty(3 * int(eo[-1]) + 3, np.uint64).fill(0)
    eng.paf_call_events(batch, svlen, snp, ev_cnt=cnt, ev=ev, ev_off=ev_off)
    names, vr = bytearray(b"#"), np.zeros(n, dtype=VCF_REC_DTYPE)
    t_pool, t_offs = _pool([r[8] for r in recs])
    q_pool, q_offs = _pool([r[9] for r in recs])
    for i, r in enumerate(recs):
        tn, qn = r[2].encode(), r[3].encode()
        while len(names) % 16 == 0:
            names += b"#"
        t_at = len(names)
        names += tn + b"#"
        while len(names) % 16 == 0:
            names += b"#"
        q_at = len(names)
        names += qn + b"##"
        vr[i] = (t_at, q_at, len(tn), len(qn), r[4], r[5], r[6], r[7], t_offs[i], len(r[8]), q_offs[i], len(r[9]))
    names += b"\0"
    d_recs, d_names = eng.upload(vr), eng.upload(np.frombuffer(bytes(names), dtype=np.uint8))
    d_t, d_q = eng.upload(t_pool), eng.upload(q_pool)
    args = (batch, svlen, ev, ev_off, d_recs, d_names, d_t, d_q)
    nbytes = eng.empty(n, np.uint64).fill(0xFF)
    err = eng.empty(n, VCF_ERR_DTYPE).fill(0x5A)
    eng.paf_call_vcf(*args, nbytes=nbytes, err=err)
    off = eng.exclusive_scan_u64(n, nbytes).numpy()
    n_text = int(off[-1])
    assert n_text < (1 << 40), "count pass: %r" % (nbytes.numpy()[:8],)
    front = guard + shift
    out_off = off + np.uint64(front)
    text = eng.empty(front + n_text + guard, np.uint8).fill(GUARD_BYTE)
    eng.paf_call_vcf(*args, out=text, out_off=eng.upload(out_off))
    eng.sync()
    return nbytes.numpy(), err.numpy(), out_off, text.numpy(), ev.numpy(), eo, np.diff(op_off.astype(np.int64))


def run_k16(eng, recs, svlen, snp, guard, shift=0):
    """-> (nbytes, err, out_off, the whole buffer)"""
    return run_k16_full(eng, recs, svlen, snp, guard, shift)[:4]


def packed_index(eng, cg, tok):
    """the packed op that token `tok` of the CIGAR begins at: the tokens themselves unless the packer split a length"""
    toks = TOKEN.findall(cg)
    if all(int(x[:-1]) <= OP_MAX_LEN for x in toks[:tok]):
        return tok
    return sum(len(eng.pack_cigar(x)[0]) for x in toks[:tok])


def check_k16(eng, recs, svlen, snp, shift=0, tag=None, expect=None):
    """every record of the call against expect_record: nbytes, the text bytes, err.kind, err.ch (the raw byte when the record
    holds exactly one byte outside ACGTNacgtn) and err.item (0 for the <INV> row, else 1 + the index of the failing op's event
    in K7's list; a clean record has item == ~0, kind == 0 and ch == 0); both guards as they were.
    -> [(expectation, items of the record, item of its error or None)]"""
    exp = expect if expect is not None else [expect_record(r, svlen, snp) for r in recs]
    guard = sum(healed_len(r, svlen, snp, len(e["text"]), e["kind"] == 0) for r, e in zip(recs, exp)) + 67
    nbytes, err, out_off, buf, ev, eo, n_ops = run_k16_full(eng, recs, svlen, snp, guard, shift)
    where = (tag, svlen, snp, shift)
    out = []
    for i, (r, e) in enumerate(zip(recs, exp)):
        n_ev = int(eo[i + 1] - eo[i])
        assert int(nbytes[i]) == len(e["text"]), (where, i, "nbytes", int(nbytes[i]), len(e["text"]), err[i])
        assert int(err[i]["kind"]) == e["kind"], (where, i, "kind", err[i], e["ch"])
        item = None
        if e["kind"]:
            if e["op"] < 0:
                item = 0
            else:
                at = packed_index(eng, r[0], e["op"])
                idx = [int(x) for x in ev[3 * int(eo[i]):3 * int(eo[i + 1]):3]]
                assert at in idx, (where, i, "the failing op has no event", at, idx[:8])
                item = 1 + idx.index(at)
            assert int(err[i]["item"]) == item, (where, i, "item", err[i], item)
            got = int(err[i]["ch"])
            if e["kind"] == 2:
                odd = [x for x in r[8] + r[9] if x not in b"ACGTNacgtn"]
                if len(odd) == 1:
                    assert chr(odd[0]).upper() == e["ch"], (where, i, "the case's one bad byte is not the oracle's")
                    assert got == odd[0], (where, i, "ch", got, odd[0])
                else:
                    assert 0 < got < 128 and chr(got).upper() == e["ch"], (where, i, "ch", got, e["ch"])
            else:
                assert got == 0, (where, i, "ch", err[i])
        else:
            assert int(err[i]["item"]) == NONE and int(err[i]["ch"]) == 0, (where, i, err[i])
        out.append((e, 1 + n_ev, item))
    a, z = guard + shift, int(out_off[-1])
    assert z + guard == len(buf)
    front = np.flatnonzero(buf[:a] != GUARD_BYTE)
    back = np.flatnonzero(buf[z:] != GUARD_BYTE)
    assert not len(front), (where, "front guard", len(front), "bytes changed, the last at", int(front[-1]) - a)
    assert not len(back), (where, "back guard", len(back), "bytes changed, up to", int(back[-1]) + 1, "behind the text")
    for i, e in enumerate(exp):
        got = buf[int(out_off[i]):int(out_off[i + 1])].tobytes()
        if got != e["text"]:
            d = next((k for k in range(len(got)) if got[k] != e["text"][k]), len(got))
            assert False, (where, i, "text differs at byte", d, got[max(0, d - 60):d + 60], e["text"][max(0, d - 60):d + 60])
    return out


# ---- 1. step edges ---------------------------------------------------------------------------------------------------------
EVENT_COUNTS = (0, 1, 62, 63, 64, 65, 127, 128, 129, 1000)
EDGE_AT = (62, 63, 64, 126, 127, 128)


def check_event_counts(eng, neg):
    """records of a given number of events: item 0 shifts the steps by one, so the same events meet the step borders at other
    places on the two strands (both carry item 0; only a '-' record's holds a row)"""
    recs = [mk(snp_ops(n) + [("=", 5)], neg=neg, seed=n, q_name="q%d" % n) for n in EVENT_COUNTS]
    res = check_k16(eng, recs, 0, True, tag=("event counts", neg))
    assert [r[1] - 1 for r in res] == list(EVENT_COUNTS)
    assert all(r[0]["kind"] == 0 for r in res)


def edge_records(kind):
    """an INS row, a DEL row or an X op of 1, 2 or 70 columns as event 62, 63, 64, 126, 127, 128: the last item of a step and the
    first item of the next, on both strands"""
    mid = {"I": [("I", 5)], "D": [("D", 5)], "X1": [("X", 1)], "X2": [("X", 2)], "X70": [("X", 70)]}[kind]
    out = []
    for at in EDGE_AT:
        for neg in (False, True):
            ops = snp_ops(at) + [("=", 3)] + mid + snp_ops(4) + [("=", 2), ("D", 7), ("=", 2)]
            out.append((mk(ops, neg=neg, seed=at, t_name="c%d" % at, alpha=b"ACGTacgtNn"), at))
    return out


def check_edges(eng, kind):
    pairs = edge_records(kind)
    res = check_k16(eng, [p[0] for p in pairs], 2, True, tag=("edges", kind))
    for (rec, at), r in zip(pairs, res):
        assert r[0]["kind"] == 0 and r[1] == 1 + at + 1 + 4 + 1, (kind, at, r[1])


# ---- 2. text paths ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def sized_step_record(nbytes, neg=False):
    """one record of three events (X of 40 columns, an insertion, one more X) whose single step is exactly `nbytes` bytes of
    text with `snp` and svlen 0: the insertion's length tunes it, the oracle says when it fits"""
    m = 1
    for _ in range(40):
        r = mk([("X", 40), ("=", 3), ("I", m), ("=", 2), ("X", 1)], neg=neg, seed=7, t_name="t" * 11, q_name="q" * 7,
               t_start=10 ** 6, q_start=10 ** 6)
        have = len(orc.call_within_var_paf(r[2], r[3], "cg:Z:" + r[0], r[8], r[9], r[4], r[5], r[6], r[7], neg, True, 0))
        if have == nbytes:
            return r
        m += nbytes - have
        assert m > 0
    raise AssertionError("no insertion length gives %d bytes" % nbytes)


def check_sized_step(eng, nbytes, shift):
    """a single step of 8 191, 8 192 (the LDS stage, WGA_VCF_TB, to the byte) and 8 193 bytes (written in place); with the shifts
    0 .. 15 the text begins at every place of a 16-byte group and the stage holds up to 15 + 8 192 bytes"""
    res = check_k16(eng, [sized_step_record(nbytes)], 0, True, shift=shift, tag=("sized", nbytes))
    assert len(res[0][0]["text"]) == nbytes and res[0][1] == 4


def four_step_ops(at=90, n=200, what=("D", 9000)):
    """n events; event `at` is a long indel (its step is written in place), the others X ops of one column"""
    return snp_ops(at) + [("=", 3), what] + snp_ops(n - at - 1) + [("=", 4)]


def text_path_records():
    mixed = b"ACGTacgtNn"
    every = []
    for k in range(10):        # a 9 000-base indel every 20 events: every step of the record is written in place
        every += snp_ops(19) + [("=", 3), (("D", "I")[k % 2], 9000)]
    return [
        mk(four_step_ops(), seed=1, alpha=mixed),                             # staged, in place, staged, staged
        mk(four_step_ops(), seed=2, alpha=mixed, neg=True, t_name="T" * 40),
        mk(four_step_ops(what=("I", 9000)), seed=3, neg=True),
        mk([("=", 4), ("X", 300), ("=", 2)], seed=4, alpha=mixed),             # one lane's rows above the stage on their own
        mk(snp_ops(70) + [("=", 1), ("X", 300), ("=", 2)] + snp_ops(70), seed=5, neg=True),
        mk(every + [("=", 3)], seed=6, alpha=mixed),
        mk(every + [("=", 3)], seed=7, neg=True),
    ]


def check_text_paths(eng):
    recs = text_path_records()
    res = check_k16(eng, recs, 50, True, tag="text paths")
    assert [r[1] for r in res] == [201, 201, 201, 2, 142, 201, 201] and all(r[0]["kind"] == 0 for r in res)
    assert len(res[3][0]["text"]) > 8192
    for r in (recs[0], recs[5]):
        check_k16(eng, [r], 50, True, shift=5, tag="text paths, alone")


# ---- 3. record counts and empties ------------------------------------------------------------------------------------------
def count_records():
    """'+' records without events (no text) at both ends and between records with text, a '-' record without events (only the
    <INV> row), `20=` alone, a record whose walk K7 stops at an N op"""
    none = mk([("=", 30), ("I", 2), ("=", 4)], seed=1)                   # svlen 2: no event
    inv = mk([("=", 30), ("D", 2), ("=", 4)], seed=2, neg=True)
    return [none, mk(pattern_ops(40), seed=3), none, inv, mk([("=", 20)], seed=4), mk(pattern_ops(150), seed=5, neg=True),
            mk([("=", 3), ("X", 2), ("=", 2), ("N", 7), ("X", 3), ("I", 9), ("=", 2)], seed=6),
            mk([("=", 20)], seed=7, neg=True), none]


def check_record_counts(eng, n):
    """four waves a workgroup: the last workgroup's waves without a record leave at once"""
    recs = count_records()
    res = check_k16(eng, recs[:n], 2, True, tag=("count", n))
    res += check_k16(eng, recs[-n:], 2, True, tag=("count, from the end", n))
    assert all(r[0]["kind"] == 0 for r in res)
    if n == 9:
        assert [r[1] for r in res[:9]] == [1, 21, 1, 1, 1, 76, 2, 1, 1], [r[1] for r in res[:9]]
        assert [len(r[0]["text"]) > 0 for r in res[:9]] == [False, True, False, True, False, True, True, True, False]


# ---- 4. names and numbers --------------------------------------------------------------------------------------------------
def number_records():
    mixed = b"ACGTacgtNn"
    ops = [("=", 3), ("X", 14), ("=", 2), ("I", 6), ("=", 5), ("D", 51), ("=", 3), ("I", 3), ("=", 1), ("D", 1), ("=", 2), ("X", 2)]
    big = 9_999_999_990                     # the rows' positions pass 9 999 999 999 inside the X op
    return [mk(ops, seed=1, alpha=mixed, t_name="c", q_name="q"),
            mk(ops, seed=2, alpha=mixed, t_name="T" * 200, q_name="Q" * 200, neg=True),
            mk(ops, seed=3, alpha=mixed, t_start=big, q_start=17),
            mk(ops, seed=4, alpha=mixed, t_start=5, q_start=big - 1, neg=True),
            mk(ops, seed=5, alpha=mixed, t_start=big, q_start=big + 2, neg=True),
            mk(ops, seed=6, alpha=mixed, t_start=(1 << 32) - 8, q_start=(1 << 32) - 5),
            mk(ops, seed=7, alpha=mixed, t_start=10 ** 19 - 9, q_start=3, neg=True),        # 19 -> 20 digits inside the X op
            mk(ops, seed=8, alpha=mixed, t_start=99, q_start=10 ** 19 - 6)]


def check_names_and_numbers(eng, svlen):
    res = check_k16(eng, number_records(), svlen, True, tag="numbers")
    assert all(r[0]["kind"] == 0 for r in res)
    if svlen == 0:
        text = res[6][0]["text"]
        assert b"\t9999999999999999999\t" in text and b"\t10000000000000000000\t" in text
        assert b"\t9999999999\t" in res[2][0]["text"] and b"\t10000000000\t" in res[2][0]["text"]
    if svlen == 5:
        check_k16(eng, number_records(), svlen, False, tag="numbers, no snp")


# ---- 5. errors, one bad byte or one short sequence by construction ---------------------------------------------------------
def error_cases():
    """(name, record, (snp, svlen), kind or None, step or None).  `step`: the 64-item step the error's item lies in; checked
    against the event list, so a case cannot drift into another path"""
    P = pattern_ops(400)                    # 200 events; with snp and svlen 0 event e is op 2 e + 1 and item e + 1
    base, negb = mk(P, seed=11), mk(P, seed=12, neg=True)
    on = (True, 0)
    t_, q_ = (lambda i: adv(P, i)[0]), (lambda i: adv(P, i)[1])
    # op 8 k + 1: X of 2, + 3: I of 4, + 5: D of 4, + 7: X of 3
    X0, I0, D0 = 1, 3, 5                    # in the first step
    X1, I1, D1 = 8 * 20 + 1, 8 * 20 + 3, 8 * 20 + 5   # events 80 .. 82: the second step
    I1n, D1n = 8 * 32 + 3, 8 * 32 + 5       # without snp (two events every eight ops): events 64 and 65, the second step
    XB = snp_ops(70) + [("=", 5), ("X", 70), ("=", 5)]
    xb = mk(XB, seed=13)
    F = four_step_ops()                     # event 90 (a 9 000-base deletion) makes step 1 an in-place step
    fs = mk(F, seed=14)
    cases = [
        ("the <INV> row's base", put(negb, "t", 0, ord("U")), (False, 0), 2, 0),
        ("an X column's REF", put(base, "t", t_(X0) + 1, ord("*")), on, 2, 0),
        ("an X column's ALT", put(base, "q", q_(X0), ord("d")), on, 2, 0),
        ("an X column's REF in a later step", put(negb, "t", t_(X1), ord("R")), on, 2, 1),
        ("an X column's ALT in a later step", put(base, "q", q_(X1 + 6) + 2, ord("k")), on, 2, 1),
        ("column 0 of a 70-column X op", put(xb, "t", adv(XB, 141)[0], ord("H")), on, 2, 1),
        ("column 40 of a 70-column X op", put(xb, "q", adv(XB, 141)[1] + 40, ord("V")), on, 2, 1),
        ("the base in front of an INS", put(base, "t", t_(I0) - 1, ord("R")), (False, 2), 2, 0),
        ("the base in front of an INS in a later step", put(negb, "q", q_(I1n) - 1, ord("y")), (False, 2), 2, 1),
        ("the base in front of a DEL", put(base, "q", q_(D0) - 1, ord("r")), (False, 3), 2, 0),
        ("the base in front of a DEL in a later step", put(base, "t", t_(D1n) - 1, ord("S")), (False, 3), 2, 1),
        ("inside an insertion's ALT", put(base, "q", q_(I1) + 2, ord("k")), on, 2, 1),
        ("inside a deletion's REF", put(negb, "t", t_(D1) + 3, ord("Y")), on, 2, 1),
        ("inside a deletion's REF in the first step", put(base, "t", t_(D0) + 1, ord("W")), (False, 1), 2, 0),
        ("lane 57", put(base, "t", t_(2 * 56 + 1), ord("M")), on, 2, 0),
        ("the last item of the first step", put(base, "t", t_(2 * 62 + 1), ord("B")), on, 2, 0),
        ("the first item of the second step", put(base, "q", q_(2 * 63 + 1), ord("D")), on, 2, 1),
        ("the last event of a record", put(base, "q", q_(399) + 2, ord("W")), on, 2, 3),
        ("in a step written in place, behind the long row", put(fs, "t", adv(F, 2 * 100 + 1)[0], ord("R")), on, 2, 1),
        ("in a step written in place, in front of the long row", put(fs, "q", adv(F, 2 * 70 + 1)[1], ord("K")), on, 2, 1),
        ("inside the long deletion's REF", put(fs, "t", adv(F, 181)[0] + 5000, ord("V")), on, 2, 1),
        ("in the step behind one written in place", put(with_neg(fs, True), "t", adv(F, 2 * 140 + 1)[0], ord("R")), on, 2, 2),
        # slices: one base short
        ("target short of an X column", cut(base, "t", t_(X0) + 1), on, 1, 0),
        ("query short of an X column", cut(negb, "q", q_(X1) + 1), on, 1, 1),
        ("target short of an X column in a later step", cut(base, "t", t_(X1 + 6) + 2), on, 1, 1),
        ("query short of an INS", cut(base, "q", q_(I0) + 3), on, 1, 0),
        ("target short of an INS", cut(negb, "t", t_(I1n) - 1), (False, 2), 1, 1),
        ("query short of an INS in a later step", cut(base, "q", q_(I1n) + 3), (False, 3), 1, 1),
        ("target short of a DEL", cut(base, "t", t_(D0) + 3), (False, 0), 1, 0),
        ("target short of a DEL in a later step", cut(negb, "t", t_(D1) + 3), on, 1, 1),
        ("query short of a DEL", cut(base, "q", q_(D1n) - 1), (False, 1), 1, 1),
        ("target short of the long deletion", cut(fs, "t", adv(F, 181)[0] + 8999), on, 1, 1),
        # two errors: the earlier item is reported
        ("a bad base in front of a short target, one step", cut(put(base, "t", t_(X0), ord("R")), "t", t_(D0 + 8) + 3), on, 2, 0),
        ("a short query in front of a bad base, one step", put(cut(base, "q", q_(I0) + 3), "t", t_(X0 + 16), ord("R")), on, 1, 0),
        ("a bad base in front of a short target, two steps", cut(put(negb, "q", q_(X0 + 8), ord("m")), "t", t_(D1) + 3), on, 2, 0),
        ("a short target a step behind a bad base", put(cut(base, "t", t_(D1) + 3), "q", q_(X0), ord("R")), on, 2, 0),
        ("a short target in a step in front of a bad base's", put(cut(base, "t", t_(D0) + 3), "q", q_(X1), ord("R")), on, 1, 0),
        ("a bad base and a short query on neighbouring lanes", cut(put(base, "t", t_(X1), ord("R")), "q", q_(I1) + 3), on, 2, 1),
        ("a short query and a bad base on neighbouring lanes", put(cut(base, "q", q_(I1) + 3), "t", t_(D1) + 2, ord("R")), on, 1, 1),
        # places that raise nothing
        ("an X column without snp", put(base, "t", t_(X1), ord("R")), (False, 0), None, None),
        ("an indel of exactly svlen bases", put(base, "q", q_(I1) + 1, ord("R")), (True, 4), None, None),
        ("a deletion of exactly svlen bases", put(negb, "t", t_(D1) + 1, ord("R")), (False, 4), None, None),
        ("an '=' column no row quotes", put(put(base, "t", t_(X1 + 1) + 1, ord("R")), "q", q_(X1 + 1) + 1, ord("R")), on, None, None),
    ]
    R2 = snp_ops(66) + [("=", 3), ("I", 5), ("D", 5), ("=", 3)] + snp_ops(70)
    cases.append(("an indel behind an indel", put(mk(R2, seed=16), "t", adv(R2, 134)[0] + 2, ord("R")), on, None, None))
    R3 = [("D", 6), ("I", 4)] + snp_ops(140)
    cases.append(("an indel at the record's start", put(put(mk(R3, seed=17), "t", 3, ord("R")), "q", 1, ord("Y")), on, None, None))
    return cases


def neighbours():
    return [mk(pattern_ops(100), seed=21, neg=True, t_name="n1"), mk(pattern_ops(180), seed=22, neg=True, q_name="n2")]


def check_error_case(eng, case, arrangements=("single", "first", "middle", "last")):
    """the case's record alone, and as the first, the middle and the last of three with clean '-' neighbours (the four waves of
    a workgroup write their records' text side by side)"""
    name, rec, (snp, svlen), kind, step = case
    e = expect_record(rec, svlen, snp)
    assert (e["kind"] or None) == kind, (name, "the case does not do what it was built for", e["kind"], e["ch"], e["op"])
    n1, n2 = neighbours()
    for arr in arrangements:
        recs = {"single": [rec], "first": [rec, n1, n2], "middle": [n1, rec, n2], "last": [n1, n2, rec]}[arr]
        res = check_k16(eng, recs, svlen, snp, tag=(name, arr))
        r = res[{"single": 0, "first": 0, "middle": 1, "last": 2}[arr]]
        assert (None if r[2] is None else r[2] // 64) == step, (name, "built for step", step, "item", r[2])
        assert sum(x[0]["kind"] != 0 for x in res) == (kind is not None)


def check_two_bad_records(eng):
    """each bad record reports its own error; the clean ones between and behind them are complete"""
    cases = {c[0]: c for c in error_cases()}
    n1, n2 = neighbours()
    a, b = cases["inside an insertion's ALT"][1], cases["target short of a DEL in a later step"][1]
    c = cases["in a step written in place, behind the long row"][1]
    # the last two share their target's and their query's slice in the pools
    res = check_k16(eng, [n1, a, n2, with_neg(n1, False), b, c, n2, with_neg(n2, False)], 0, True, tag="two bad records")
    assert [r[0]["kind"] for r in res] == [0, 2, 0, 0, 1, 2, 0, 0]


# ---- 6. an indel no sequence has moved in front of, an empty target, split indels ------------------------------------------
ZERO_CASES = [("0=5I9=", True, 1), ("0=5I9=", False, 1), ("3I0=4D9=", True, 1), ("0X5I9=", True, 2), ("0X5I9=", False, 1),
              ("0X4D9=", True, 2), ("0M6D2=", False, 1), ("3=1X2=0I4=", True, None), ("4D0=5I9=", True, 1)]


def check_zero_length_op(eng, case):
    """a zero-length M-like op in front of an indel: after_m is set, no base lies in front, the reference's slice start
    underflows and the slice panics.  (cigar, snp, item or None)"""
    cg, snp, item = case
    for neg in (False, True):
        rec = (cg, neg, "chrT", "qry", 100, 120, 200, 220, b"ACGTACGTACGTACGTACGTA", b"TGCATGCATGCATGCATGCAT")
        n1, n2 = neighbours()
        for recs, at in (([rec], 0), ([n1, rec, n2], 1)):
            res = check_k16(eng, recs, 0, snp, tag=("zero-length", cg, neg))
            e, _, got = res[at]
            assert got == item and e["kind"] == (1 if item else 0), (cg, snp, neg, e, got)
            if item:
                assert e["text"].count(b"\n") == int(neg)       # no text from that event on


def check_empty_target(eng):
    """a '-' record whose fetched target is empty: kind 1 at item 0 and no text (the oracle: byte index 1 out of range).  The
    slice lies inside the pool, between other records' slices"""
    n1, n2 = neighbours()
    full = mk(pattern_ops(40), seed=31, neg=True)
    empty = full[:8] + (b"",) + full[9:]
    for recs, at in (([empty], 0), ([n1, empty, n2], 1), ([n1, n2, empty], 2), ([empty, n1], 0)):
        res = check_k16(eng, recs, 0, True, tag="empty target")
        e, _, item = res[at]
        assert e["kind"] == 1 and item == 0 and e["text"] == b""
    res = check_k16(eng, [with_neg(empty, False)], HUGE, False, tag="empty target, '+'")     # no row asks for a base
    assert res[0][0]["kind"] == 0


SPLIT = (1 << 28) + 4     # 268 435 460: packed as an op of 2^28 - 1 and a continuation piece of 5


def check_split_indel(eng, op):
    """`5=268435460D5=` / `...I...`: the sum of the op and its continuation piece decides `len > svlen` and the slice check.
    Error path only: a clean row of that length is left out on purpose.  One lane writes an indel row byte by byte, so a row
    of 2^28 bytes would take far longer than a test may; how long has not been measured."""
    cg = "5=%d%s5=" % (SPLIT, op)
    assert [int(w) & 15 for w in eng.pack_cigar(cg)[0]] == [7, {"D": 2, "I": 1}[op], {"D": 10, "I": 9}[op], 7]
    n1, n2 = neighbours()
    for neg in (False, True):
        rec = (cg, neg, "chrT", "qry", 100, 130, 200, 230, b"ACGTACGTACGTACGTACGTA", b"TGCATGCATGCATGCATGCAT")
        for svlen, kind in ((SPLIT - 1, 1), (SPLIT, 0), (0, 1)):
            for recs, at in (([rec], 0), ([n1, rec, n2], 1)):
                res = check_k16(eng, recs, svlen, True, tag=("split", op, neg, svlen))
                e, items, item = res[at]
                assert e["kind"] == kind and item == (1 if kind else None) and items == 2, (op, neg, svlen, e, items, item)
                assert e["text"].count(b"\n") == int(neg)


# ---- 7. the random battery -------------------------------------------------------------------------------------------------
# shares of = / X / I / D ops, the longest '=' op, the longest of the others
DENSITIES = [((0.50, 0.20, 0.15, 0.15), 40, 12), ((0.50, 0.30, 0.10, 0.10), 80, 6), ((0.40, 0.20, 0.20, 0.20), 6, 4),
             ((0.50, 0.10, 0.20, 0.20), 12, 60)]


def synth_records(seed, n, density, max_ops=3000):
    p, max_m, max_g = density
    rng = np.random.default_rng(seed)
    out = []
    for k in range(n):
        n_ops = int(rng.integers(1, max_ops + 1))
        kinds = rng.choice(4, size=n_ops, p=list(p))
        lens = np.where(kinds == 0, rng.integers(1, max_m + 1, n_ops), rng.integers(1, max_g + 1, n_ops))
        ops = [("=XID"[c], int(ln)) for c, ln in zip(kinds, lens)]
        out.append(mk(ops, neg=bool(rng.integers(0, 2)), seed=seed * 1000 + k, t_name="chrT%d" % (k % 3), q_name="qry.%d" % (k % 2),
                      t_start=int(rng.integers(0, 10 ** 6)), q_start=int(rng.integers(0, 10 ** 6)), alpha=b"ACGTacgtN"))
    return out


def spoil(recs, seed, share):
    """about `share` of the records get one IUPAC byte or lose their target's or query's tail, at the larger of two draws: the
    first error of a record should often lie many items in"""
    rng = np.random.default_rng(seed)
    out = []
    for r in recs:
        if rng.random() < share:
            row = "tq"[int(rng.integers(0, 2))]
            n = len(r[8 if row == "t" else 9])
            pos = int(max(rng.integers(0, n, 2)))
            r = put(r, row, pos, IUPAC[int(rng.integers(0, len(IUPAC)))]) if rng.random() < 0.5 else cut(r, row, pos)
        out.append(r)
    return out


def check_random_battery(eng, seeds, n_recs=10, bad_share=0.5):
    """records of 1 .. 3 000 ops at four densities and both strands, half of them spoilt; svlen from SVLENS in turn, `snp` off
    for one seed in five.
    -> (records, records of more than one step, bad records, bad records whose error lies behind the first step)"""
    tot = multi = nbad = late = 0
    for k, seed in enumerate(seeds):
        svlen, snp = SVLENS[k % 4], k % 5 != 3
        recs = spoil(synth_records(seed, n_recs, DENSITIES[k % len(DENSITIES)]), seed + 1, bad_share)
        for e, items, item in check_k16(eng, recs, svlen, snp, tag=("random", seed)):
            tot += 1
            multi += items > 64
            nbad += e["kind"] != 0
            late += item is not None and item >= 64
    return tot, multi, nbad, late


def assert_battery_shares(tot, multi, nbad, late):
    """the random battery must not go trivial: MOST records take more than one 64-item step, a quarter and more of the records
    are bad, and a GOOD PART (a quarter and more) of the bad records have their error behind the first step: there the fill
    pass has clean steps in hand and must end exactly where the count pass did.
    Measured: the emulator suite (seeds 100 .. 114, 10 records each) has 150 records, 136 of more than one step, 44 bad, 39 of them
    behind the first step; the GPU suite (seeds 1000 .. 1059, 24 each) 1 440 records, 1 321, 429 and 357."""
    assert 2 * multi > tot, (multi, tot)
    assert 4 * nbad >= tot, (nbad, tot)
    assert 4 * late >= nbad, (late, nbad)
