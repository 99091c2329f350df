"""The MAF record frames of `paf2maf` and `chain2maf` on the device (K32): the C-ABI entry (Engine.maf_frame, Engine.maf_records)
against maf_frame_ref (the restatement from maf.rs) around the oracle's rows, against wga_paf2maf_layout for the places, and
the two commands with their device writer against WGA_MAF_FRAME_WRITER=host and the expected text.
Imported by test_emu_maf_frame.py (emulator build, CPU) and test_gpu_maf_frame.py (the product on a GPU); each provides the
`cli` and `eng` fixtures."""
import ctypes as C
import gzip
import random

import numpy as np

import maf2paf_cases as m2p
import maf_frame_ref as ref
import oracle_py as orc
import parity_cases as pc
from chain_split_cases import run, write
from wgatools_amd.engine import COUNTS_DTYPE, DIAG_DTYPE, MAF_FRAME_HEAD_DTYPE

U64 = (1 << 64) - 1
E_INVALID_ARG = -1
GUARD = 64
CIGARS = ("3M", "2I4M1D3M2D", "1D2I5=1X1I")
BASES = b"ACGTacgtNn"


# ---- records and arrays ----------------------------------------------------------------------------------------------------------
def seq(n, k=0):
    return bytes(BASES[(7 * i + 3 * k + i // 5) % 10] for i in range(n))


def rec(cg="3M", neg=False, tname=b"tchr", qname=b"qchr", score=60, t=(100, 10 ** 9), q=(700, 10 ** 9), t_neg=False, k=0,
        t_seq=None, q_seq=None):
    """a record: the CIGAR text, the query's strand, the names, the score, t / q = (start, source size) as printed (the aligned
    size printed is the slice's length), and the two fetched slices (what the CIGAR consumes unless they are given)"""
    tl, ql = pc.consumption(cg)
    t_seq = seq(tl, k) if t_seq is None else t_seq
    q_seq = seq(ql, k + 1) if q_seq is None else q_seq
    return dict(cg=cg, neg=neg, tname=tname, qname=qname, score=score, t=(t[0], len(t_seq), t[1]), q=(q[0], len(q_seq), q[1]),
                t_neg=t_neg, t_seq=t_seq, q_seq=q_seq)


def some(n, k0=0):
    """n records over CIGARS on both strands, with names and numbers of several widths"""
    return [rec(CIGARS[(k + k0) % 3], neg=(k + k0) % 2 == 1, tname=b"t" * (1 + k % 5), qname=b"q%d" % (k % 11), score=k % 61,
                t=(10 ** (k % 7), 2 * 10 ** 9), q=(7 * k, 10 ** 9 + k), k=k) for k in range(n)]


def heads_of(recs):
    """(names, heads): the names back to back in one buffer, one wga_maf_frame_head per record"""
    names = bytearray()
    heads = np.zeros(len(recs) + 1, dtype=MAF_FRAME_HEAD_DTYPE)
    for r, b in enumerate(recs):
        h = heads[r]
        h["score"], h["t"], h["q"] = b["score"], b["t"], b["q"]
        h["t_neg"], h["q_neg"] = 1 if b["t_neg"] else 0, 1 if b["neg"] else 0
        h["tname_off"], h["tname_len"] = len(names), len(b["tname"])
        names += b["tname"]
        h["qname_off"], h["qname_len"] = len(names), len(b["qname"])
        names += b["qname"]
    return bytes(names), heads


def ref_heads(recs, names=None):
    """the restatement's two heads of every record; `names` = the (tname, qname) the spans stand for when they were edited"""
    out = []
    for r, b in enumerate(recs):
        tn, qn = names[r] if names else (b["tname"], b["qname"])
        out.append((ref.t_head(b["score"], tn, b["t"], b["t_neg"]), ref.q_head(qn, b["q"], b["neg"])))
    return out


class Arrays:
    """wga_paf2maf_frame's arrays for a list of records.  K1's part is wga_cigar_stat on the packed CIGARs (with the pools the
    row kernel reads), or hand-built: rows = (t_src_len, inserted bases, q_src_len, deleted bases) per record, and bad =
    {record: the field of its diagnostic that is set}"""

    def __init__(self, eng, recs, rows=None, bad=None):
        self.eng, self.recs, self.n = eng, recs, len(recs)
        self.names, self.heads = heads_of(recs)
        n = self.n
        if rows is None:
            b = pc.batch_from_texts(eng, [r["cg"] for r in recs], [1 if r["neg"] else 0 for r in recs],
                                    [r["t_seq"] for r in recs], [r["q_seq"] for r in recs])
            self.b = b
            self.batch = eng.make_batch(b["ops"], b["op_off"], b["strand_neg"])
            self.d_counts, self.d_diag, self.tile_ws = eng.cigar_stat(self.batch)
            c = self.d_counts.numpy()
            self.t_rows = [int(b["t_src_len"][r]) + int(c[r]["ins_bp"]) + int(c[r]["inv_ins_bp"]) for r in range(n)]
            self.q_rows = [int(b["q_src_len"][r]) + int(c[r]["del_bp"]) + int(c[r]["inv_del_bp"]) for r in range(n)]
            self.d_tl, self.d_ql = eng.upload(b["t_src_len"]), eng.upload(b["q_src_len"])
            self.d_to, self.d_qo = eng.upload(b["t_src_off"]), eng.upload(b["q_src_off"])
            self.d_tp, self.d_qp = eng.upload(b["t_pool"]), eng.upload(b["q_pool"])
            self.diags = None                                                    # the row kernel's: known after it ran
        else:
            self.batch = None
            counts = np.zeros(n + 1, dtype=COUNTS_DTYPE)
            tl, ql = np.zeros(n + 1, dtype=np.uint64), np.zeros(n + 1, dtype=np.uint64)
            for r, (a, ins, c, dele) in enumerate(rows):
                tl[r], ql[r] = a, c
                counts[r]["ins_bp"], counts[r]["inv_ins_bp"] = ins - ins // 3, ins // 3      # both terms of a row's length
                counts[r]["del_bp"], counts[r]["inv_del_bp"] = dele - dele // 3, dele // 3
            self.t_rows, self.q_rows = [a + ins for a, ins, _, _ in rows], [c + dele for _, _, c, dele in rows]
            diag = np.full(3 * (n + 1), U64, dtype=np.uint64).view(DIAG_DTYPE)
            for r, field in (bad or {}).items():
                diag[r][field] = r % 5
            self.diags = [tuple(int(v) for v in g) for g in diag[:n]]
            self.d_counts, self.d_diag, self.d_tl, self.d_ql = eng.upload(counts), eng.upload(diag), eng.upload(tl), eng.upload(ql)
        self.upload()

    def upload(self):
        self.d_names = self.eng.upload(np.frombuffer(self.names + b"\0" * 16, dtype=np.uint8))
        self.d_heads = self.eng.upload(self.heads)

    def args(self):
        return self.n, self.d_names, len(self.names), self.d_heads, self.d_counts, self.d_tl, self.d_ql

    def layout(self, names=None):
        hd = ref_heads(self.recs, names)
        return ref.layout([len(t) for t, _ in hd], self.t_rows, [len(q) for _, q in hd], self.q_rows)

    def frames_text(self, names=None, gap=b"\xa5"):
        """the text a fill of the frames alone leaves in a buffer of 0xA5: every record's, bad or not"""
        return b"".join(t + gap * self.t_rows[r] + q + gap * self.q_rows[r] + ref.TAIL for r, (t, q) in enumerate(ref_heads(self.recs, names)))

    def n_good(self):
        return ref.n_good(self.diags)


def oracle_rows(recs):
    """(the two rows of every record in front of the first one the oracle refuses, that record's error or None): the record
    loop of converter.rs:219-235 — the query slice reverse-complemented on '-', then parse_cigar_to_insert"""
    out = []
    for b in recs:
        try:
            q = orc.reverse_complement(b["q_seq"]) if b["neg"] else b["q_seq"]
            out.append(orc.parse_cigar_to_insert("cg:Z:" + b["cg"], b["t_seq"], q))
        except orc.OracleError as e:
            return out, e
    return out, None


def expected_text(recs, rows):
    """the restatement's frames around the oracle's rows of the leading records"""
    return b"".join(t + rows[r][0] + q + rows[r][1] + ref.TAIL for r, (t, q) in enumerate(ref_heads(recs[:len(rows)])))


def check_records(eng, recs, shift=0, error_kind=None):
    """Engine.maf_records (K1, K32 count, the row kernel, K32 fill; the guards around the text are checked inside) gives the
    expected text in front of the first record the oracle refuses, and that record's index"""
    a = Arrays(eng, recs)
    got, good, whole = eng.maf_records(a.batch, a.names, a.heads, a.d_tp, len(a.b["t_pool"]), a.d_to, a.d_tl, a.d_qp,
                                       len(a.b["q_pool"]), a.d_qo, a.d_ql, out_shift=shift)
    rows, err = oracle_rows(recs)
    assert (err.kind if err else None) == error_kind, (err and err.message, error_kind)
    assert good == len(rows), (good, len(rows))
    want = expected_text(recs, rows)
    assert got == want, (shift, len(got), len(want), got[:200], want[:200])
    assert len(whole) == a.layout()[2][-1] and whole.startswith(want)
    return got, whole, a


def check_frames(eng, a, names=None, shift=0, null_names=False, no_diag=False):
    """Engine.maf_frame on hand-built arrays: the restatement's frames, 0xA5 where the rows belong, the places of the rows and
    the records, n_good and good_bytes"""
    n, d_names, nnb, heads, counts, tl, ql = a.args()
    if null_names:
        d_names, nnb = None, 0
    got, good, good_bytes, lay = eng.maf_frame(n, d_names, nnb, heads, counts, tl, ql, diag=None if no_diag else a.d_diag,
                                               out_shift=shift)
    want = a.frames_text(names)
    assert got == want, (shift, len(got), len(want), got[:200], want[:200])
    t_off, q_off, rec_off = a.layout(names)
    assert [int(v) for v in lay[0].numpy()[:n]] == t_off and [int(v) for v in lay[1].numpy()[:n]] == q_off
    assert [int(v) for v in lay[2].numpy()] == rec_off and rec_off[-1] == len(want)
    want_good = n if no_diag else a.n_good()
    assert (good, good_bytes) == (want_good, rec_off[want_good]), (good, good_bytes, want_good, rec_off[want_good])
    return got


# ---- ABI level -----------------------------------------------------------------------------------------------------------------
COUNTS = (1, 2, 3, 4, 5, 63, 64, 65, 255, 256, 257, 1025)


def check_abi_record_counts(eng, counts=COUNTS):
    """one record, a block of the fill (4), a wave, a block of the plan (256), the scan's tile (1024), and one more"""
    for n in counts:
        text, _, _ = check_records(eng, some(n, n))
        assert text.count(b"a score=") == n and text.endswith(b"\n\n")


class Raw:
    """the calls of wga_paf2maf_frame and the row kernel by hand, on a buffer of 0xA5 with GUARD bytes around the text"""

    def __init__(self, eng, a, work=None):
        self.eng, self.a = eng, a
        self.work = work if work is not None else eng.empty(max(int(eng.lib.wga_paf2maf_frame_work_bytes(a.n)), 16), np.uint8)
        self.t_off, self.q_off, self.rec_off = eng.empty(a.n + 1, np.uint64), eng.empty(a.n + 1, np.uint64), eng.empty(a.n + 2, np.uint64)
        self.total = eng.maf_frame_count(*a.args(), self.work, self.t_off, self.q_off, self.rec_off, diag=a.d_diag)
        self.out = eng.upload(np.full(self.total + 2 * GUARD + 16, 0xA5, dtype=np.uint8))

    def fill_frames(self):
        a, tot, good, gb = self.a, C.c_uint64(self.total), C.c_uint32(0), C.c_uint64(0)
        n, names, nb, heads, counts, tl, ql = a.args()
        rc = self.eng.lib.wga_paf2maf_frame(self.eng.ctx, n, names.ptr, nb, heads.ptr, counts.ptr, tl.ptr, ql.ptr, a.d_diag.ptr,
                                            self.work.ptr, self.t_off.ptr, self.q_off.ptr, self.rec_off.ptr, C.byref(tot),
                                            C.byref(good), C.byref(gb), self.out.ptr + GUARD)
        assert rc == 0 and tot.value == self.total
        self.eng.sync()
        return good.value, gb.value

    def fill_rows(self):
        a = self.a
        self.eng.paf2maf_expand(a.batch, a.d_counts, a.tile_ws, a.d_tp, len(a.b["t_pool"]), a.d_to, a.d_tl, a.d_qp,
                                len(a.b["q_pool"]), a.d_qo, a.d_ql, self.out.ptr + GUARD, self.t_off, self.q_off, a.d_diag)
        self.eng.sync()

    def text(self):
        got = self.out.numpy()
        assert (got[:GUARD] == 0xA5).all() and (got[GUARD + self.total:] == 0xA5).all(), "a byte outside d_out[0 .. total)"
        return got[GUARD:GUARD + self.total].tobytes()


def check_abi_either_order(eng):
    """K32's fill alone leaves every row byte as it was and writes every frame byte; the row kernel alone leaves every frame
    byte as it was; in either order the two give the expected text"""
    recs = some(70, 1)
    rows, err = oracle_rows(recs)
    assert err is None
    want = expected_text(recs, rows)
    a = Arrays(eng, recs)
    frames_only = a.frames_text()
    rows_only = bytes(w if f == 0xA5 else 0xA5 for w, f in zip(want, frames_only))
    assert len(frames_only) == len(want) and frames_only.count(b"\xa5") == sum(a.t_rows) + sum(a.q_rows)
    x = Raw(eng, a)
    assert x.total == len(want)
    assert x.fill_frames() == (70, len(want))
    assert x.text() == frames_only
    x.fill_rows()
    assert x.text() == want
    y = Raw(eng, a)
    y.fill_rows()
    assert y.text() == rows_only
    assert y.fill_frames() == (70, len(want))
    assert y.text() == want


def check_abi_alignment(eng):
    """target heads and query heads that between them start at every offset within a 16-byte group; d_out at every offset
    behind an aligned address"""
    recs = [rec(CIGARS[k % 3], neg=k % 2 == 1, tname=b"t" * (1 + k % 7), qname=b"q" * (k % 3), k=k) for k in range(48)]
    a = Arrays(eng, recs)
    t_off, q_off, rec_off = a.layout()
    hd = ref_heads(recs)
    starts = {v % 16 for v in rec_off[:-1]} | {(q_off[r] - len(hd[r][1])) % 16 for r in range(48)}
    assert starts == set(range(16)), starts
    for shift in range(16):
        check_records(eng, recs, shift=shift)


def check_abi_empty_rows(eng):
    """hand-built counts and source lengths: an empty target row (the two heads are adjacent), an empty query row (the query
    head is adjacent to the record's end), and both"""
    recs = some(9)
    rows = [(5, 2, 4, 1), (0, 0, 6, 2), (3, 0, 0, 0), (0, 0, 0, 0), (0, 0, 0, 0), (7, 1, 0, 0), (0, 0, 3, 0), (0, 0, 0, 0), (2, 2, 2, 2)]
    for shift in (0, 5, 15):
        text = check_frames(eng, Arrays(eng, recs, rows=rows), shift=shift)
        assert b"\t2000000000\t\ns\tq3\t" in text and b"\t1000000003\t\n\na score=4\n" in text
    assert check_frames(eng, Arrays(eng, recs[:1], rows=[(0, 0, 0, 0)])).endswith(b"\t\ns\tq0\t0\t3\t+\t1000000000\t\n\n")


def check_abi_names(eng):
    """names of 0, 1, 15, 16 and 17 bytes and of 7 000 (over the stage: written directly); a tab, a quote and a byte that is
    not ASCII go out as they are; a span outside the names and a null d_names are empty names"""
    special = 'a\tb"cé'.encode()
    for name in (b"", b"n", b"n" * 15, b"n" * 16, b"n" * 17, special, b"N" * 7000):
        for recs in ([rec(CIGARS[1]), rec(CIGARS[2], qname=name, neg=True), rec(CIGARS[0])],
                     [rec(CIGARS[1], tname=name), rec(CIGARS[0], tname=name, qname=name)]):
            text, _, _ = check_records(eng, recs)
            assert b"s\t" + name + b"\t" in text and len(text) > len(name)
    # spans outside the names: behind the end, across the end, an offset of 2^64 - 1; a span that ends at the end is inside
    recs = some(4)
    rows = [(3, 0, 2, 1), (0, 0, 0, 0), (5, 5, 5, 5), (1, 0, 0, 0)]
    a = Arrays(eng, recs, rows=rows)
    nb = len(a.names)
    a.heads[0]["qname_off"], a.heads[0]["qname_len"] = nb, 1
    a.heads[1]["tname_off"], a.heads[1]["tname_len"] = nb - 2, 3
    a.heads[2]["qname_off"], a.heads[2]["qname_len"] = U64, 4
    a.heads[2]["tname_off"], a.heads[2]["tname_len"] = 1 << 40, 0xFFFFFFFF
    a.heads[3]["tname_off"], a.heads[3]["tname_len"] = nb - 3, 3
    a.upload()
    names = [(recs[0]["tname"], b""), (b"", recs[1]["qname"]), (b"", b""), (a.names[-3:], recs[3]["qname"])]
    text = check_frames(eng, a, names=names)
    assert text.startswith(b"a score=0\ns\tt\t1\t3\t+\t2000000000\t\xa5\xa5\xa5\ns\t\t0\t3\t+\t1000000000\t")
    # d_names == NULL with n_name_bytes == 0: every span is outside
    check_frames(eng, a, names=[(b"", b"")] * 4, null_names=True)


VALUES = (0, 9, 10, 10 ** 19 - 1, 10 ** 19, U64)


def check_abi_values(eng):
    """every one of the seven printed numbers at the widths' borders, and both strand letters on both lines"""
    recs = []
    for v in VALUES:
        for field in range(7):
            b = rec(t_neg=(field + len(recs)) % 2 == 1, neg=(field // 2 + len(recs)) % 2 == 1)
            nums = [b["score"]] + list(b["t"]) + list(b["q"])
            nums[field] = v
            b["score"], b["t"], b["q"] = nums[0], tuple(nums[1:4]), tuple(nums[4:7])
            recs.append(b)
    recs.append(rec(score=U64, t=(U64, U64), q=(U64, U64), t_neg=True, neg=True))
    recs[-1]["t"], recs[-1]["q"] = (U64,) * 3, (U64,) * 3
    a = Arrays(eng, recs, rows=[(k % 4, k % 3, k % 5, k % 2) for k in range(len(recs))])
    text = check_frames(eng, a, shift=3)
    for letters in (b"\t+\t", b"\t-\t"):
        assert any(letters in t for t, _ in ref_heads(recs)) and any(letters in q for _, q in ref_heads(recs))
    for v in VALUES:                                                              # the score, a start, an aligned size, a source size
        assert b"a score=%d\n" % v in text and b"\ttchr\t%d\t3\t" % v in text and b"\tqchr\t700\t%d\t" % v in text
        assert b"\t+\t%d\t" % v in text or b"\t-\t%d\t" % v in text
    big = b"%d" % U64
    assert b"a score=" + big + b"\ns\ttchr\t" + big + b"\t" + big + b"\t-\t" + big + b"\t" in text


def random_rows(rnd, n):
    return [(rnd.choice((0, 1, 17, 4000, 10 ** 6)), rnd.choice((0, 0, 3, 999)), rnd.choice((0, 2, 16, 65536)), rnd.choice((0, 1, 70)))
            for _ in range(n)]


def check_abi_layout_equivalence(eng, seeds=range(4)):
    """on random batches the count call's three arrays are wga_paf2maf_layout's for pre_t / pre_q = the restatement's head
    lengths and post = 2, and the Python-integer layout's"""
    for seed in seeds:
        rnd = random.Random(700 + seed)
        n = (1, 260, 1024, 1500)[seed % 4]
        recs = [rec(tname=b"t" * rnd.randrange(0, 30), qname=b"q" * rnd.randrange(0, 30), score=rnd.choice(VALUES),
                    t=(rnd.randrange(10 ** rnd.randrange(1, 19)), rnd.choice(VALUES)), q=(rnd.choice(VALUES), 5), neg=rnd.random() < 0.5)
                for _ in range(n)]
        a = Arrays(eng, recs, rows=random_rows(rnd, n))
        x = Raw(eng, a)
        hd = ref_heads(recs)
        pre_t = eng.upload(np.array([len(t) for t, _ in hd], dtype=np.uint32))
        pre_q = eng.upload(np.array([len(q) for _, q in hd], dtype=np.uint32))
        post = eng.upload(np.full(n, 2, dtype=np.uint32))
        lt, lq, lr = eng.paf2maf_layout(n, a.d_counts, a.d_tl, a.d_ql, pre_t, pre_q, post)
        got = (x.t_off.numpy()[:n], x.q_off.numpy()[:n], x.rec_off.numpy()[:n + 1])
        assert (got[0] == lt.numpy()).all() and (got[1] == lq.numpy()).all() and (got[2] == lr.numpy()).all(), seed
        want = a.layout()
        assert [[int(v) for v in g] for g in got] == [want[0], want[1], want[2]], seed
        assert x.total == want[2][-1]


def far_arrays(eng):
    """three records with 3 * 10^9 inserted bases each: the places leave 32 bits behind the first record"""
    return Arrays(eng, some(3), rows=[(1000, 3 * 10 ** 9, 10, 7), (0, 3 * 10 ** 9, 5 * 10 ** 9, 3 * 10 ** 9), (77, 3 * 10 ** 9, 1, 0)])


def check_abi_far_places_count(eng):
    """count only: places beyond 2^32, compared with Python integers"""
    a = far_arrays(eng)
    x_work = eng.empty(max(int(eng.lib.wga_paf2maf_frame_work_bytes(3)), 16), np.uint8)
    t_off, q_off, rec_off = eng.empty(4, np.uint64), eng.empty(4, np.uint64), eng.empty(5, np.uint64)
    total = eng.maf_frame_count(*a.args(), x_work, t_off, q_off, rec_off)
    want = a.layout()
    assert total == want[2][-1] > 17 * 10 ** 9 and want[1][1] > 1 << 32 and want[2][2] > 1 << 33
    assert [int(v) for v in t_off.numpy()[:3]] == want[0] and [int(v) for v in q_off.numpy()[:3]] == want[1]
    assert [int(v) for v in rec_off.numpy()[:4]] == want[2]


def check_abi_far_places_fill(eng):
    """fill (a GPU's memory): two records whose second has its frames beyond 4 GiB, in one buffer of 4 GiB + 64 KiB set to 0xA5
    on the device; only the windows around the frames and the guards come back"""
    recs = [rec(tname=b"first", qname=b"one", score=1), rec(tname=b"second.beyond.4GiB", qname=b"two", score=2, neg=True)]
    size = (4 << 30) + (64 << 10)
    hd = ref_heads(recs)
    fixed = sum(len(t) + len(q) for t, q in hd) + 4
    t0 = (4 << 30) + 1000 - len(hd[0][0])                                          # the first target row ends behind 4 GiB
    rows = [(t0, 0, 300, 11), (5000, 7, 40000, 0)]
    a = Arrays(eng, recs, rows=rows, bad={1: "panic_op_idx"})
    t_off, q_off, rec_off = a.layout()
    total = rec_off[-1]
    assert total == fixed + t0 + 311 + 5007 + 40000 and rec_off[1] > 1 << 32 and total + 2 * GUARD + 16 <= size
    work = eng.empty(max(int(eng.lib.wga_paf2maf_frame_work_bytes(2)), 16), np.uint8)
    lay = eng.empty(2, np.uint64), eng.empty(2, np.uint64), eng.empty(3, np.uint64)
    assert eng.maf_frame_count(*a.args(), work, *lay, diag=a.d_diag) == total
    out = eng.empty(size, np.uint8).fill(0xA5)
    lead = GUARD + 5                                                               # not 16-byte aligned
    tot, good, gb = C.c_uint64(total), C.c_uint32(0), C.c_uint64(0)
    n, names, nb, heads, counts, tl, ql = a.args()
    rc = eng.lib.wga_paf2maf_frame(eng.ctx, n, names.ptr, nb, heads.ptr, counts.ptr, tl.ptr, ql.ptr, a.d_diag.ptr, work.ptr,
                                   lay[0].ptr, lay[1].ptr, lay[2].ptr, C.byref(tot), C.byref(good), C.byref(gb), out.ptr + lead)
    assert rc == 0 and (good.value, gb.value) == (1, rec_off[1])
    eng.sync()
    assert [int(v) for v in lay[2].numpy()] == rec_off

    def window(lo, hi):                                                            # text bytes [lo, hi)
        return eng.download_slice(out, lead + lo, hi - lo).tobytes()
    assert window(-lead, 0) == b"\xa5" * lead                                      # the guard in front
    assert window(0, t_off[0] + 64) == hd[0][0] + b"\xa5" * 64
    assert window(t_off[0] + t0 - 64, q_off[0] + 64) == b"\xa5" * 64 + hd[0][1] + b"\xa5" * 64
    end0 = q_off[0] + 311
    assert window(end0 - 64, t_off[1] + 64) == b"\xa5" * 64 + ref.TAIL + hd[1][0] + b"\xa5" * 64
    assert window(t_off[1] + 5007 - 64, q_off[1] + 64) == b"\xa5" * 64 + hd[1][1] + b"\xa5" * 64
    assert window(total - 66, total) == b"\xa5" * 64 + ref.TAIL
    assert window(total, total + 4096) == b"\xa5" * 4096                          # the guard behind
    assert eng.download_slice(out, size - 4096, 4096).tobytes() == b"\xa5" * 4096


def check_abi_bad_records_by_hand(eng, sizes=(9, 300, 1030)):
    """hand-built diagnostics: each of the three fields at the first, the middle and the last record, and behind a block of the
    plan and a tile of the scan; n_good and good_bytes are the restatement's, and the frames behind the cut are written"""
    for n in sizes:
        recs = some(n)
        rows = [((k * 7) % 23 if k % 5 else 0, k % 3, (k * 5) % 19, k % 2) for k in range(n)]
        spots = (0, n // 2, n - 1) if n < 100 else (n - 3,)
        for at in spots:
            for field in DIAG_DTYPE.names:
                a = Arrays(eng, recs, rows=rows, bad={at: field, n - 1: "bad_op_idx"})
                assert a.n_good() == at
                check_frames(eng, a)
    a = Arrays(eng, some(9), rows=[(1, 1, 1, 1)] * 9, bad={6: "bad_base_pos", 3: "panic_op_idx"})
    assert a.n_good() == 3
    check_frames(eng, a)
    check_frames(eng, a, no_diag=True)                                           # d_diag == NULL: no record is bad


def check_abi_bad_records_pipeline(eng):
    """through K1 and the row kernel: an `N` op, a CIGAR that inserts beyond its slice, an invalid base on a '-' record; the
    text in front of the cut is the expected text"""
    for at in (0, 4, 8):
        for kind, bad in ((2, rec("5M3N2M", k=1)), (6, rec("10=2I3=", t_seq=seq(5), k=2)),
                          (4, rec("4=1X3=", neg=True, q_seq=b"ACGZACGT", k=3))):
            recs = some(9, 2)
            recs[at] = bad
            text, whole, a = check_records(eng, recs, error_kind=kind)
            assert text.count(b"a score=") == at and whole.count(b"a score=") == 9      # the frames behind the cut are written
    recs = some(9, 2)                                                             # two bad records: the first one cuts
    recs[6], recs[3] = rec("5M3N2M"), rec("4=", neg=True, q_seq=b"AC!T")
    assert check_records(eng, recs, error_kind=4)[0].count(b"a score=") == 3


def raw(eng, a, n=None, work=True, null=(), names_bytes=None, total=True, good=True, good_bytes=True):
    d_work = eng.empty(max(int(eng.lib.wga_paf2maf_frame_work_bytes(a.n)), 16), np.uint8)
    lay = eng.empty(a.n + 1, np.uint64), eng.empty(a.n + 1, np.uint64), eng.empty(a.n + 2, np.uint64)
    tot, gd, gb = C.c_uint64(7), C.c_uint32(7), C.c_uint64(7)
    p = dict(names=a.d_names.ptr, heads=a.d_heads.ptr, counts=a.d_counts.ptr, tl=a.d_tl.ptr, ql=a.d_ql.ptr, diag=a.d_diag.ptr,
             t_off=lay[0].ptr, q_off=lay[1].ptr, rec_off=lay[2].ptr)
    for k in null:
        p[k] = None
    rc = eng.lib.wga_paf2maf_frame(eng.ctx, a.n if n is None else n, p["names"], len(a.names) if names_bytes is None else names_bytes,
                                   p["heads"], p["counts"], p["tl"], p["ql"], p["diag"], d_work.ptr if work else None, p["t_off"],
                                   p["q_off"], p["rec_off"], C.byref(tot) if total else None, C.byref(gd) if good else None,
                                   C.byref(gb) if good_bytes else None, None)
    return rc, tot.value, gd.value


def check_abi_arguments(eng):
    recs = some(3)
    a = Arrays(eng, recs)
    rows, _ = oracle_rows(recs)
    want = expected_text(recs, rows)
    assert raw(eng, a) == (0, len(want), 3)
    for n in (None, 0):                                                           # whatever the count
        assert raw(eng, a, work=False, n=n)[0] == E_INVALID_ARG
        assert raw(eng, a, total=False, n=n)[0] == E_INVALID_ARG and raw(eng, a, good=False, n=n)[0] == E_INVALID_ARG
        assert raw(eng, a, good_bytes=False, n=n)[0] == E_INVALID_ARG
    for null in ("names", "heads", "counts", "tl", "ql", "t_off", "q_off", "rec_off"):
        assert raw(eng, a, null=(null,))[0] == E_INVALID_ARG, null
        assert raw(eng, a, n=0, null=(null,)) == (0, 0, 0), null
    assert raw(eng, a, null=("diag",)) == (0, len(want), 3)                       # d_diag may be null
    assert raw(eng, a, null=("names",), names_bytes=0)[:1] == (0,)                # d_names is checked only when it has bytes
    assert raw(eng, a, n=0) == (0, 0, 0)                                          # n == 0: total 0, n_good 0
    assert eng.maf_frame(0, None, 0, None, None, None, None)[:3] == (b"", 0, 0)
    assert int(eng.lib.wga_paf2maf_frame_work_bytes(0)) == 8 * (2 * 0 + 2 + 0 // 1024 + 4)     # the documented formula
    assert int(eng.lib.wga_paf2maf_frame_work_bytes(5000)) == 8 * (2 * 5000 + 2 + 5000 // 1024 + 4)
    # count and fill take the same arguments (Raw); a second fill after the first gives the same bytes
    x = Raw(eng, a)
    x.fill_rows()
    assert x.fill_frames() == (3, len(want))
    once = x.text()
    assert x.fill_frames() == (3, len(want))
    assert x.text() == once == want
    # a workspace that another batch used before
    b = Arrays(eng, some(2, 1))
    y = Raw(eng, b, work=x.work)
    y.fill_frames()
    y.fill_rows()
    assert y.text() == expected_text(b.recs, oracle_rows(b.recs)[0])


def random_recs(seed, n=None):
    rnd = random.Random(5000 + seed)
    n = n or 40 + (seed * 67) % 261
    recs = []
    for k in range(n):
        cg = "".join("%d%s" % (rnd.choice((1, 1, 2, 9, 10, 33)), rnd.choice("M=XIDM")) for _ in range(rnd.randrange(1, 9)))
        recs.append(rec(cg, neg=rnd.random() < 0.5, tname=b"ref.chr%d" % rnd.randrange(25), qname=b"qry.ctg%d" % rnd.randrange(40),
                        score=rnd.randrange(256), t=(rnd.randrange(10 ** 9), 10 ** 9 + rnd.randrange(10 ** 9)),
                        q=(rnd.randrange(10 ** 9), 10 ** 9 + rnd.randrange(10 ** 9)), k=k))
    return recs


def check_abi_random(eng, seeds=range(12)):
    for seed in seeds:
        recs = random_recs(seed)
        kind = None
        if seed % 4 == 3:
            recs[len(recs) * 2 // 3] = rec("12=5N3=")
            kind = 2
        check_records(eng, recs, shift=seed % 16, error_kind=kind)


# ---- command level -----------------------------------------------------------------------------------------------------------------
HOST_WRITER = {"WGA_MAF_FRAME_WRITER": "host"}


def both_writers(cli, *args, env=None, to=None):
    """the command under the device writer and under WGA_MAF_FRAME_WRITER=host: the same bytes (of stdout, or of the file `to`
    that -o names), exit status and message, and under WGA_TIMING=1 the phase named after the writer that ran"""
    env = env or {}
    cmd = [a for a in args if a in ("paf2maf", "chain2maf")][0]
    args = list(args) + (["-o", to, "-r"] if to else [])
    res = []
    for e in (env, dict(env, **HOST_WRITER)):
        rc, out, msg, timing = m2p.timed(cli, args, e)
        res.append((rc, open(to, "rb").read() if to else out, msg, timing))
    dev, host = res
    assert dev[0] in (0, 1) and dev[:3] == host[:3], (args, dev[0], host[0], dev[2], host[2], dev[1][-200:], host[1][-200:])
    assert "%s records (device)" % cmd in dev[3] and "%s records (host)" % cmd not in dev[3], dev[3]
    assert "%s records (host)" % cmd in host[3] and "%s records (device)" % cmd not in host[3], host[3]
    return dev[:3]


T_CONTIGS = ((b"tchr", 5000), (b"t.long_contig_name_17", 3000), (b"t", 4100))
Q_CONTIGS = ((b"qchr", 4500), (b"q2", 3900))


def fasta(contigs, k0):
    seqs = {name: seq(size, k0 + j) for j, (name, size) in enumerate(contigs)}
    text = b"".join(b">" + name + b" description\n" + b"".join(s[i:i + 60] + b"\n" for i in range(0, len(s), 60))
                    for name, s in seqs.items())
    return seqs, text


def paf_case(tmp_path, seed, n):
    """(paf path, target FASTA path, query FASTA path, records): records over several contigs whose slices are cut from the FASTAs"""
    rnd = random.Random(9000 + seed)
    tseqs, ttext = fasta(T_CONTIGS, 0)
    qseqs, qtext = fasta(Q_CONTIGS, 5)
    recs = []
    for k in range(n):
        cg = "".join("%d%s" % (rnd.choice((1, 2, 9, 10, 33)), rnd.choice("M=XIDM")) for _ in range(rnd.randrange(1, 12)))
        cg = "%d=" % rnd.randrange(1, 20) + cg                                    # both slices have bases: the fetch of an empty range is not the subject
        tl, ql = pc.consumption(cg)
        (tn, tsize), (qn, qsize), neg = T_CONTIGS[k % 3], Q_CONTIGS[k % 2], rnd.random() < 0.5
        ts, qs = rnd.randrange(tsize - tl), rnd.randrange(qsize - ql)
        b = rec(cg, neg=neg, tname=tn, qname=qn, score=rnd.randrange(61), t=(ts, tsize), q=(qsize - (qs + ql) if neg else qs, qsize),
                t_seq=tseqs[tn][ts:ts + tl], q_seq=qseqs[qn][qs:qs + ql])
        b["paf_q"] = (qs, qs + ql)
        recs.append(b)
    return recs, write(tmp_path, "t.fa", ttext), write(tmp_path, "q.fa", qtext)


def paf_text(recs):
    return b"".join(b"%s\t%d\t%d\t%d\t%s\t%s\t%d\t%d\t%d\t0\t0\t%d\tcg:Z:%s\n" % (
        b["qname"], b["q"][2], b["paf_q"][0], b["paf_q"][1], b"-" if b["neg"] else b"+", b["tname"], b["t"][2], b["t"][0],
        b["t"][0] + b["t"][1], b["score"], b["cg"].encode()) for b in recs)


def maf_text(kind, t_fa, q_fa, recs, upto=None):
    rows, _ = oracle_rows(recs[:upto])
    return b"#maf version=1.6 convert_from=%s t_seq_path=%s q_seq_path=%s\n" % (kind, t_fa.encode(), q_fa.encode()) + expected_text(recs, rows)


def check_cli_paf2maf(cli, tmp_path):
    recs, t_fa, q_fa = paf_case(tmp_path, 1, 60)
    want = maf_text(b"paf", t_fa, q_fa, recs)
    paf = write(tmp_path, "r.paf", paf_text(recs))
    assert both_writers(cli, "paf2maf", paf, "-g", t_fa, "-q", q_fa) == (0, want, "")
    assert both_writers(cli, "paf2maf", paf, "-g", t_fa, "-q", q_fa, to=str(tmp_path / "o.maf")) == (0, want, "")
    gz = str(tmp_path / "o.maf.gz")                                               # a .gz output: equal after inflating
    for env in ({}, HOST_WRITER):
        rc, _, err = run(cli, "paf2maf", paf, "-g", t_fa, "-q", q_fa, "-o", gz, "-r", env=env)
        assert rc == 0 and gzip.open(gz, "rb").read() == want, err


def check_cli_paf2maf_host_reader(cli, tmp_path):
    """the host PAF reader, and a PAF with a quoted name on one line (a piece the host reader takes)"""
    recs, t_fa, q_fa = paf_case(tmp_path, 2, 40)
    want = maf_text(b"paf", t_fa, q_fa, recs)
    text = paf_text(recs)
    assert both_writers(cli, "paf2maf", write(tmp_path, "h.paf", text), "-g", t_fa, "-q", q_fa, env={"WGA_PAF_READER": "host"}) == (0, want, "")
    lines = text.split(b"\n")
    assert lines[7].startswith(recs[7]["qname"] + b"\t")
    lines[7] = b'"' + recs[7]["qname"] + b'"' + lines[7][len(recs[7]["qname"]):]
    assert both_writers(cli, "paf2maf", write(tmp_path, "q.paf", b"\n".join(lines)), "-g", t_fa, "-q", q_fa) == (0, want, "")


def check_cli_paf2maf_pieces(cli, tmp_path):
    """several pieces; an invalid op in the middle of the second piece ends the text in front of its record; a tokeniser error"""
    recs, t_fa, q_fa = paf_case(tmp_path, 5, 90)
    text = paf_text(recs)
    chunk = len(text) // 4
    assert chunk > 500
    paf = write(tmp_path, "p.paf", text)
    want = maf_text(b"paf", t_fa, q_fa, recs)
    assert both_writers(cli, "paf2maf", paf, "-g", t_fa, "-q", q_fa, env={"WGA_CHUNK_BYTES": str(chunk)}) == (0, want, "")
    at, bad = 0, None
    for r, line in enumerate(text.split(b"\n")[:-1]):                             # the record over the middle byte of the second piece
        if at <= chunk + chunk // 2 < at + len(line) + 1:
            bad = r
        at += len(line) + 1
    assert 10 < bad < 80
    good_cg = recs[bad]["cg"]
    recs[bad]["cg"] = good_cg + "3N"
    paf = write(tmp_path, "b.paf", paf_text(recs))
    want = maf_text(b"paf", t_fa, q_fa, recs, upto=bad)
    for env in ({}, {"WGA_CHUNK_BYTES": str(chunk)}):
        assert both_writers(cli, "paf2maf", paf, "-g", t_fa, "-q", q_fa, env=env) == (1, want, "CIGAR OP `N` invalid"), env
    recs[bad]["cg"] = good_cg + "7"                                               # a number without an op: the tokeniser's error
    rc, out, msg = both_writers(cli, "paf2maf", write(tmp_path, "t.paf", paf_text(recs)), "-g", t_fa, "-q", q_fa)
    assert rc == 1 and out == want and msg != ""


def chain_case(tmp_path, seed, n, t_neg_at=()):
    """(records, target FASTA path, query FASTA path): chains whose data lines are (size, dt, dq), slices fetched forward"""
    rnd = random.Random(9500 + seed)
    tseqs, ttext = fasta(T_CONTIGS, 2)
    qseqs, qtext = fasta(Q_CONTIGS, 9)
    recs = []
    for k in range(n):
        lines = [(rnd.randrange(1, 40), rnd.randrange(3) * rnd.randrange(8), rnd.randrange(3) * rnd.randrange(8)) for _ in range(rnd.randrange(1, 9))]
        lines[-1] = (lines[-1][0], 0, 0)
        tl, ql = sum(s + dt for s, dt, _ in lines), sum(s + dq for s, _, dq in lines)
        (tn, tsize), (qn, qsize), neg = T_CONTIGS[k % 3], Q_CONTIGS[k % 2], rnd.random() < 0.5
        ts, qs = rnd.randrange(tsize - tl), rnd.randrange(qsize - ql)
        recs.append(dict(lines=lines, neg=neg, t_neg=k in t_neg_at, tname=tn, qname=qn, score=255, t=(ts, tl, tsize),
                         q=(qsize - (qs + ql) if neg else qs, ql, qsize), chain_q=(qs, qs + ql), t_seq=tseqs[tn][ts:ts + tl],
                         q_seq=qseqs[qn][qs:qs + ql]))
    return recs, write(tmp_path, "ct.fa", ttext), write(tmp_path, "cq.fa", qtext)


def chain_text(recs):
    out = []
    for k, b in enumerate(recs):
        out.append(b"chain %d %s %d %s %d %d %s %d %s %d %d %d\n" % (1000 + k, b["tname"], b["t"][2], b"-" if b["t_neg"] else b"+", b["t"][0],
                                                                     b["t"][0] + b["t"][1], b["qname"], b["q"][2], b"-" if b["neg"] else b"+",
                                                                     b["chain_q"][0], b["chain_q"][1], k + 1))
        out += [b"%d\t%d\t%d\n" % ln for ln in b["lines"][:-1]] + [b"%d\n\n" % b["lines"][-1][0]]
    return b"".join(out)


def chain_maf_text(t_fa, q_fa, recs, upto=None):
    rows = []
    for b in recs[:upto]:
        q = orc.reverse_complement(b["q_seq"]) if b["neg"] else b["q_seq"]
        rows.append(orc.parse_chain_to_insert(b["lines"], b["t_seq"], q))
    return b"#maf version=1.6 convert_from=chain t_seq_path=%s q_seq_path=%s\n" % (t_fa.encode(), q_fa.encode()) + expected_text(recs, rows)


def check_cli_chain2maf(cli, tmp_path):
    """a plain chain file, the host reader, a '-' target strand, a failing record in the middle"""
    recs, t_fa, q_fa = chain_case(tmp_path, 3, 50, t_neg_at=(4, 17))
    want = chain_maf_text(t_fa, q_fa, recs)
    assert want.count(b"\t-\t%d\t" % recs[4]["t"][2]) >= 1
    ch = write(tmp_path, "r.chain", chain_text(recs))
    assert both_writers(cli, "chain2maf", ch, "-g", t_fa, "-q", q_fa) == (0, want, "")
    assert both_writers(cli, "chain2maf", ch, "-g", t_fa, "-q", q_fa, env={"WGA_CHAIN_READER": "host"}) == (0, want, "")
    # record 23's lines put a gap behind the end of its slices: String::insert_str panics in the reference
    b = recs[23]
    b["lines"] = b["lines"][:-1] + [(b["lines"][-1][0] + 5, 3, 0), (1, 0, 0)]
    rc, out, msg = both_writers(cli, "chain2maf", write(tmp_path, "b.chain", chain_text(recs)), "-g", t_fa, "-q", q_fa)
    assert rc == 1 and "panic" in msg and out == chain_maf_text(t_fa, q_fa, recs, upto=23)


def check_cli_gpus(cli, tmp_path, gpus=2):
    """--gpus N into a file: every device writes its records' frames; the bytes of one device, also in front of a failing record"""
    recs, t_fa, q_fa = paf_case(tmp_path, 6, 80)
    paf = write(tmp_path, "g.paf", paf_text(recs))
    to = str(tmp_path / "g.maf")
    one = both_writers(cli, "paf2maf", paf, "-g", t_fa, "-q", q_fa, to=to)
    assert one == (0, maf_text(b"paf", t_fa, q_fa, recs), "")
    assert both_writers(cli, "--gpus", str(gpus), "paf2maf", paf, "-g", t_fa, "-q", q_fa, to=to) == one
    recs[50]["cg"] += "3N"
    paf = write(tmp_path, "gb.paf", paf_text(recs))
    one = both_writers(cli, "paf2maf", paf, "-g", t_fa, "-q", q_fa, to=to)
    assert one == (1, maf_text(b"paf", t_fa, q_fa, recs, upto=50), "CIGAR OP `N` invalid")
    assert both_writers(cli, "--gpus", str(gpus), "paf2maf", paf, "-g", t_fa, "-q", q_fa, to=to) == one
    crecs, ct_fa, cq_fa = chain_case(tmp_path, 8, 60)
    ch = write(tmp_path, "g.chain", chain_text(crecs))
    one = both_writers(cli, "chain2maf", ch, "-g", ct_fa, "-q", cq_fa, to=to)
    assert one == (0, chain_maf_text(ct_fa, cq_fa, crecs), "")
    assert both_writers(cli, "--gpus", str(gpus), "chain2maf", ch, "-g", ct_fa, "-q", cq_fa, to=to) == one
