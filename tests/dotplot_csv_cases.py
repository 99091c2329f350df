"""The base-level csv rows of `dotplot` on the device (K26): the C-ABI entry (Engine.dotplot_csv) on hand-built segment arrays
against dotplot_csv_ref.rows_ref, K12 -> K26 against the oracle's segment lists, and the `wgatools dotplot --out-format csv`
command with the device writer against WGA_DOTPLOT_WRITER=host.
Imported by test_emu_dotplot_csv.py (emulator build, CPU) and test_gpu_dotplot_csv.py (the product on a GPU); each provides the
`cli` and `eng` fixtures."""
import ctypes as C
import os
import random
import subprocess

import numpy as np

import dotplot_csv_ref as ref
import oracle_py as orc
import text_items_cases as ti
from helpers import GOLDEN
from wgatools_amd import synth

U64 = (1 << 64) - 1
E_INVALID_ARG = -1
ROWS = 256           # rows per block of the count and fill kernels
STAGE = ROWS * 90    # bytes of a block's text that go through LDS
SHORT = b",a,b\n"    # the shortest tail two names make


# ---- ABI level -----------------------------------------------------------------------------------------------------------------
class Rows:
    """hand-built arrays on the device: segs (rows of five u64), the segment count and the tail of every record"""

    def __init__(self, eng, segs, counts, tails):
        assert len(counts) == len(tails) and sum(counts) == len(segs)
        self.segs = [tuple(int(v) for v in s) for s in segs]
        self.off = np.cumsum([0] + list(counts)).astype(np.uint64)
        self.tails = list(tails)
        self.n = len(counts)
        self.d_segs = eng.upload(np.array(self.segs, dtype=np.uint64).reshape(-1))      # no segment: an allocation all the same
        self.d_off = eng.upload(self.off)
        self.d_tails = eng.upload(np.frombuffer(b"".join(self.tails) + b"\0", dtype=np.uint8))
        self.d_tail_off = eng.upload(np.cumsum([0] + [len(t) for t in self.tails]).astype(np.uint64))
        self.want = ref.rows_ref(self.segs, self.off, self.tails)

    def args(self):
        return self.n, self.d_segs, self.d_off, self.d_tails, self.d_tail_off


def check(eng, segs, counts, tails, shift=0, rows=None):
    """the device's bytes are the restatement's; the guards around d_out are checked inside Engine.dotplot_csv"""
    rows = rows or Rows(eng, segs, counts, tails)
    text = eng.dotplot_csv(*rows.args(), out_shift=shift)
    assert text == rows.want, (shift, len(text), len(rows.want), counts[:8], text[:120], rows.want[:120])
    return text


def seg(k, kind=None):
    """a small segment that depends on its index"""
    return (k, k + 7, 1000 * (k % 90), 1000 * (k % 90) + k % 13, k % 3 if kind is None else kind)


def segs_of(n, k0=0):
    return [seg(k0 + k) for k in range(n)]


def check_abi_block_edges(eng):
    """256 rows per block: one record of n segments, then a second record behind it — its border lies before, on and behind a
    block's border"""
    for n in (254, 255, 256, 257, 513):
        text = check(eng, segs_of(n), [n], [b",chrT,chrQ\n"])
        assert text.count(b"\n") == n
        text = check(eng, segs_of(n + 3), [n, 3], [b",chrT,chrQ\n", b",second,q\n"])
        assert text.count(b",second,q\n") == 3 and text.endswith(b",second,q\n")


def check_abi_empty_records(eng):
    """runs of records without segments at the start, in the middle, across a block's border and at the end"""
    t = [b",t%d,q%d\n" % (k, k * k) for k in range(40)]
    for counts in ([0, 0, 0, 3, 2], [4, 0, 0, 0, 1, 0, 2], [3, 2, 0, 0, 0], [0, 5, 0], [0, 0, 200, 0, 0, 56, 0, 0, 0, 5, 0, 0, 1],
                   [256, 0, 0, 0, 256, 0, 1, 0], [0] * 9 + [255, 0, 1, 0, 0, 1, 0] + [0] * 9, [1] + [0] * 30 + [1]):
        text = check(eng, segs_of(sum(counts)), counts, t[:len(counts)])
        assert text.count(b"\n") == sum(counts)
    for n in (1, 5, 300):                                                    # every record empty: 0 bytes, the guards untouched
        assert check(eng, [], [0] * n, [SHORT] * n) == b""
    assert eng.dotplot_csv(0, None, None, None, None) == b""               # n == 0
    none = Rows(eng, [], [0], [SHORT])
    assert eng.dotplot_csv(0, none.d_segs, none.d_off, none.d_tails, none.d_tail_off) == b""


def check_abi_stage_limit(eng):
    """600 rows of four times 2^64 - 1 and a 5-byte tail: 90 bytes each, 256 of them are exactly the stage"""
    text = check(eng, [(U64, U64, U64, U64, 2)] * 600, [600], [SHORT])
    assert len(text) == 600 * (4 * 20 + 5 + 5) and ROWS * 90 == STAGE
    check(eng, segs_of(2) + [(U64, U64, U64, U64, 1)] * 600 + segs_of(2), [2, 600, 2], [b",x,y\n", SHORT, b",z,w\n"])


def check_abi_over_the_stage(eng):
    """tails of 9 000 bytes (two of them in a block still fit the stage) and of 20 000 bytes (the block writes directly),
    between records with short tails; then 300 rows of a short tail, 300 of the long one, 300 of a short one"""
    for n in (9000, 20000):
        long_t, long_q = b"," + b"T" * (n - 4) + b",q\n", b",t," + b"Q" * (n - 4) + b"\n"
        assert len(long_t) == n and len(long_q) == n
        text = check(eng, segs_of(9), [3, 1, 2, 1, 2], [SHORT, long_t, b",c,d\n", long_q, b",e,f\n"])
        assert len(text) > 2 * n and (len(text) > STAGE) == (n == 20000)      # one block: staged, then direct
        check(eng, segs_of(5), [1, 4], [long_t, SHORT])
        text = check(eng, segs_of(900), [300, 300, 300], [SHORT, long_t, b",c,d\n"])
        assert len(text) > 300 * n


def check_abi_alignment(eng):
    """tails of 1 .. 33 bytes in successive one-segment records: the rows start at every offset within a 16-byte group; d_out at
    every offset behind an aligned address"""
    tails = [b"x" * k + b"\n" for k in range(33)]
    rows = Rows(eng, segs_of(33, 5), [1] * 33, tails)
    text = check(eng, None, [1] * 33, None, rows=rows)
    starts, at = set(), 0
    for line in text.split(b"\n")[:-1]:
        starts.add(at % 16)
        at += len(line) + 1
    assert at == len(text) and starts == set(range(16)), starts
    small = Rows(eng, segs_of(44), [3, 1, 40], [b",a,b\n", b",abcdefg,h\n", b",t,q\n"])
    for shift in range(16):
        check(eng, None, [3, 1, 40], None, shift=shift, rows=small)
        check(eng, None, [1] * 33, None, shift=shift, rows=rows)


def check_abi_values(eng):
    """every digit count in every field; the edges of the decimal lengths; the three kinds, and `?` for a kind above 2"""
    segs = []
    for f in range(4):
        for d in range(1, 21):
            s = [7, 7, 7, 7, d % 3]
            s[f] = 10 ** (d - 1)
            segs.append(tuple(s))
    edge = [0, 9, 10, 1 << 63, U64] + [10 ** k - 1 for k in range(1, 20)] + [10 ** k for k in range(1, 20)]
    for k, v in enumerate(edge):
        for f in range(4):
            s = [edge[(k + 1 + g) % len(edge)] for g in range(4)]
            s[f] = v
            segs.append(tuple(s) + ((k + f) % 3,))
    text = check(eng, segs, [80, len(segs) - 80], [b",t,q\n", b",u,v\n"])
    assert text.startswith(b"1,7,7,7,I,t,q\n10,7,7,7,D,t,q\n")
    got = {len(x) for line in text.split(b"\n")[:80] for x in line.split(b",")[:4]}
    assert got == set(range(1, 21))
    assert check(eng, [(0, 0, 0, 0, 0), (1, 2, 3, 4, 1), (5, 6, 7, 8, 2)], [3], [SHORT]) == b"0,0,0,0,M,a,b\n1,2,3,4,I,a,b\n5,6,7,8,D,a,b\n"
    # a kind above 2 is the caller's error and an ordinary input to the letter's lookup: `?`
    assert check(eng, [(1, 2, 3, 4, 3), (1, 2, 3, 4, 1 << 40), (1, 2, 3, 4, U64), (1, 2, 3, 4, 2)], [4], [SHORT]) == \
        b"1,2,3,4,?,a,b\n" * 3 + b"1,2,3,4,D,a,b\n"


def check_abi_opaque_tails(eng):
    """tails as the host's quoting makes them, copied byte for byte"""
    names = [(b"chr1", b"q"), (b'a"b', b"q"), (b"t,1", b'"'), (b"line\nbreak", b"cr\rname"), (b"caf\xc3\xa9", b"\xff\x80\xfe"),
             (b'"",\n\r', b""), (b"", b"x")]
    tails = [ref.tail(t, q) for t, q in names]
    assert tails[1] == b',"a""b",q\n' and tails[2] == b',"t,1",""""\n' and tails[3] == b',"line\nbreak","cr\rname"\n'
    assert tails[5] == b',""""",\n\r",\n' and tails[6] == b",,x\n"
    counts = [2, 1, 3, 2, 1, 2, 1]
    text = check(eng, segs_of(sum(counts)), counts, tails)
    for t, c in zip(tails, counts):
        assert text.count(t) >= c


def raw(eng, rows, n=None, segs=True, off=True, tails=True, tail_off=True, work=True, d_off=None, out=None, total=7):
    """one call of wga_dotplot_csv as it is; (rc, *total_bytes)"""
    n_rows = int(rows.off[-1])
    d_work = eng.empty(max(int(eng.lib.wga_dotplot_csv_work_bytes(n_rows)), 16), np.uint8) if work is True else work
    tot = C.c_uint64(total)
    rc = eng.lib.wga_dotplot_csv(eng.ctx, rows.n if n is None else n, rows.d_segs.ptr if segs else None,
                                 (rows.d_off if d_off is None else d_off).ptr if off else None, rows.d_tails.ptr if tails else None,
                                 rows.d_tail_off.ptr if tail_off else None, d_work.ptr if work else None, C.byref(tot), out)
    return rc, int(tot.value)


def check_abi_arguments(eng):
    rows = Rows(eng, segs_of(5), [3, 2], [SHORT, b",c,d\n"])
    assert raw(eng, rows) == (0, len(rows.want))
    for null in ("segs", "off", "tails", "tail_off"):
        assert raw(eng, rows, **{null: False})[0] == E_INVALID_ARG, null      # a null array with n > 0
    assert raw(eng, rows, n=0, segs=False, off=False, tails=False, tail_off=False, work=False) == (0, 0)
    assert raw(eng, rows, work=False)[0] == E_INVALID_ARG                     # a null d_work with N > 0
    empty = Rows(eng, [], [0, 0], [SHORT, SHORT])
    assert raw(eng, empty, work=False) == (0, 0)                              # ... not with N == 0
    # more than 0xFFFFFFF0 rows: the call reads the last offset and refuses before it reads a segment (there are five of them)
    assert raw(eng, rows, d_off=eng.upload(np.array([0, 3, 0xFFFFFFF1], dtype=np.uint64)))[0] == E_INVALID_ARG
    assert raw(eng, rows, d_off=eng.upload(np.array([0, 3, 1 << 40], dtype=np.uint64)))[0] == E_INVALID_ARG
    assert int(eng.lib.wga_dotplot_csv_work_bytes(0)) >= 8
    assert int(eng.lib.wga_dotplot_csv_work_bytes(31000)) == 8 * (31000 + 1 + 31000 // 1024 + 4)


def check_abi_count_fill(eng):
    """the count call alone, then fills into a buffer of a pattern: exactly total_bytes bytes change (no tail and no row holds the
    pattern's byte), and two fills from one count give the same bytes"""
    counts = [(k * 7) % 41 for k in range(60)]
    rows = Rows(eng, segs_of(sum(counts)), counts, [b",t%d,q\n" % k for k in range(60)])
    work = eng.empty(int(eng.lib.wga_dotplot_csv_work_bytes(sum(counts))), np.uint8)
    total = eng.dotplot_csv_count(*rows.args(), work)
    assert total == len(rows.want) and 0x5A not in rows.want
    fills = []
    for lead in (100, 107):
        out = eng.upload(np.full(total + 300, 0x5A, dtype=np.uint8))
        assert raw(eng, rows, work=work, out=out.ptr + lead, total=total) == (0, total)
        eng.sync()
        got = out.numpy()
        assert int((got != 0x5A).sum()) == total
        assert (got[:lead] == 0x5A).all() and (got[lead + total:] == 0x5A).all()
        fills.append(got[lead:lead + total].tobytes())
    assert fills[0] == fills[1] == rows.want
    assert eng.dotplot_csv(*rows.args(), work=work) == rows.want          # the same workspace under another pair of calls


def item_stream(eng):
    """two records of 300 rows: 600 items, three blocks of the fill.  The scan of the row sizes leads d_work: word 0
    (capi_dotplot_csv.inc)"""
    rows = Rows(eng, segs_of(600), [300, 300], [b",chrT,chrQ\n", b",second,q\n"])
    work = eng.empty(int(eng.lib.wga_dotplot_csv_work_bytes(600)), np.uint8)
    assert eng.dotplot_csv_count(*rows.args(), work) == len(rows.want)

    def fill(total_bytes, d_out):
        assert raw(eng, rows, work=work, out=d_out, total=total_bytes) == (0, total_bytes)
    return ti.Stream(eng, work, 0, 600, rows.want, fill)


def check_abi_fill_short_total(eng):
    ti.check_short_total(item_stream(eng))


def check_abi_fill_scan_one_off(eng):
    ti.check_scan_one_off(item_stream(eng), size_checked=True)


def random_rows(seed):
    """up to 2 000 records of 0 .. 40 segments, 64-bit values of a random digit count, tails of 3 .. 60 bytes"""
    rnd = random.Random(1000 + seed)
    n = (1, 17, 300, 2000)[seed % 4] if seed < 4 else rnd.randint(1, 2000)

    def value():
        d = rnd.randint(1, 20)
        return rnd.randint(0 if d == 1 else 10 ** (d - 1), min(10 ** d - 1, U64))

    counts = [rnd.choice((0, 0, 1, 2, rnd.randint(0, 40))) for _ in range(n)]
    segs = [(value(), value(), value(), value(), rnd.randint(0, 2)) for _ in range(sum(counts))]
    tails = []
    for _ in range(n):
        k = rnd.randint(3, 60)
        tails.append(b"," + bytes(rnd.choice(b"abcXYZ019_.|") for _ in range(k - 3)) + b",\n")
    return segs, counts, tails


def check_abi_random(eng, seeds):
    for seed in seeds:
        segs, counts, tails = random_rows(seed)
        assert all(3 <= len(t) <= 60 for t in tails)
        check(eng, segs, counts, tails, shift=seed % 16)


def merged_cigar(sl):
    """the cg:Z: text of packed ops, the pieces of a split I / D joined"""
    toks = []
    for w in sl.tolist():
        c, ln = w & 15, w >> 4
        if c in (9, 10) and toks:
            toks[-1][0] += ln
        else:
            toks.append([ln, synth.OP_CHARS[c] if c < 9 else "B"])
    return "cg:Z:" + "".join("%d%s" % (ln, ch) for ln, ch in toks)


def check_pipeline(eng, cutoff=3):
    """K12 -> K26: the text of the segments K12 wrote is the rows of the oracle's segment lists"""
    b = synth.make_paf_batch(91, 14, 700, 500000)
    ops, op_off, strands = b["ops"], b["op_off"], b["strand_neg"]
    n = len(op_off) - 1
    rng = np.random.default_rng(3)
    ts, qs = rng.integers(0, 10 ** 9, n).astype(np.uint64), rng.integers(0, 10 ** 9, n).astype(np.uint64)
    batch = eng.make_batch(ops, op_off, np.asarray(strands, dtype=np.uint8))
    d_ts, d_qs = eng.upload(ts), eng.upload(qs)
    cnt = eng.cigar_dotplot(batch, cutoff, d_ts, d_qs)
    off = eng.exclusive_scan_u64(n, cnt)
    segs = eng.empty((int(off.numpy()[-1]) + 1) * 5, np.uint64).fill(0x23)
    eng.cigar_dotplot(batch, cutoff, d_ts, d_qs, segs=segs, seg_off=off)
    tails = [ref.tail(b"t,%d" % i if i % 5 == 0 else b"t%d" % i, b"q%d" % (i % 3)) for i in range(n)]
    d_tails = eng.upload(np.frombuffer(b"".join(tails), dtype=np.uint8))
    d_tail_off = eng.upload(np.cumsum([0] + [len(t) for t in tails]).astype(np.uint64))
    text = eng.dotplot_csv(n, segs, off, d_tails, d_tail_off)
    want, rows = [], 0
    for i in range(n):
        sl = ops[int(op_off[i]):int(op_off[i + 1])]
        lst = orc.cigar_to_base_plotdata(merged_cigar(sl), int(ts[i]), int(qs[i]), strands[i], cutoff) if len(sl) else []
        rows += len(lst)
        want += [b"%d,%d,%d,%d,%c" % (int(s[0]), int(s[1]), int(s[2]), int(s[3]), b"MID"[int(s[4])]) + tails[i] for s in lst]
    assert rows > 2 * ROWS and text == b"".join(want)


# ---- command level -----------------------------------------------------------------------------------------------------------------
HOST = {"WGA_DOTPLOT_WRITER": "host"}
HEADER = b"ref_start,ref_end,query_start,query_end,cigar,ref_chro,query_chro\n"
DEVICE_PHASE, HOST_PHASE = "dotplot rows (device)", "dotplot rows (host)"


def run(cli, *args, env=None):
    """(exit code, stdout, stderr) with WGA_TIMING=1"""
    r = subprocess.run([cli] + list(args), stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       env=dict(os.environ, WGA_TIMING="1", **(env or {})))
    return r.returncode, r.stdout, r.stderr.decode(errors="replace")


def both_writers(cli, *args, rc=0):
    """the command with the device writer and with the host's: the same bytes and exit code, each run naming its writer"""
    dev, host = run(cli, *args), run(cli, *args, env=HOST)
    assert dev[0] == rc and host[0] == rc, (args, dev[0], host[0], dev[2], host[2])
    assert dev[1] == host[1], (args, dev[1][:300], host[1][:300])
    if rc == 0:
        assert DEVICE_PHASE in dev[2] and HOST_PHASE not in dev[2], dev[2]
        assert HOST_PHASE in host[2] and DEVICE_PHASE not in host[2], host[2]
    return dev, host


GOLDEN_RUNS = (("paf_l9", ("-f", "paf", "-l", "9", "testdotplot.paf")), ("paf_l0", ("-f", "paf", "-l", "0", "testdotplot.paf")),
               ("paf_default", ("-f", "paf", "testdotplot.paf")), ("maf_l3", ("-l", "3", "test.maf")))


def check_golden(cli, name):
    args = dict(GOLDEN_RUNS)[name]
    dev, _ = both_writers(cli, "dotplot", "--out-format", "csv", *args[:-1], os.path.join(GOLDEN, args[-1]))
    assert dev[1].startswith(HEADER) and dev[1].count(b"\n") > 2
    if name == "paf_l9":     # Appendix B's fixture: 25M10I15M20D30M20I30M10D70M from (0, 0), every indel longer than 9
        assert dev[1].startswith(HEADER + b"0,25,0,25,M,B,A\n25,25,25,35,I,B,A\n25,40,35,50,M,B,A\n40,60,50,50,D,B,A\n")


def paf_line(q, t, cg, qs=10, ts=100, neg=False):
    return ("%s\t100000\t%d\t%d\t%s\t%s\t200000\t%d\t%d\t0\t0\t60\tcg:Z:%s\n" % (q, qs, qs + 5, "-" if neg else "+", t, ts, ts + 5, cg)).encode()


def check_quoted_names(cli, tmp_path):
    """names that the csv writer quotes: once per record on the host, copied into every row on the device"""
    path = str(tmp_path / "quoted.paf")
    with open(path, "wb") as f:
        f.write(paf_line("q1", "t,1", "5=60I5=") + paf_line('q"2', "t2", "4=70D4=") + paf_line("q3", "t3", "3=") +
                paf_line('q",4', 't"",', "2=80I", neg=True))
    dev, _ = both_writers(cli, "dotplot", "-f", "paf", "--out-format", "csv", path)
    assert dev[1] == HEADER + (b'100,105,10,15,M,"t,1",q1\n105,105,15,75,I,"t,1",q1\n105,110,75,80,M,"t,1",q1\n'
                               b'100,104,10,14,M,t2,"q""2"\n104,174,14,14,D,t2,"q""2"\n174,178,14,18,M,t2,"q""2"\n'
                               b"100,103,10,13,M,t3,q3\n"
                               b'100,102,12,10,M,"t"""",","q"",4"\n102,102,92,12,I,"t"""",","q"",4"\n')


def check_no_segment(cli, tmp_path):
    """records without a segment: no row and no header line"""
    path = str(tmp_path / "none.paf")
    with open(path, "wb") as f:
        f.write(paf_line("q1", "t1", "5I") + paf_line("q2", "t2", "7D3I") + paf_line("q3", "t3", "4S"))
    dev, _ = both_writers(cli, "dotplot", "-f", "paf", "--out-format", "csv", path)
    assert dev[1] == b""
    dev, _ = both_writers(cli, "dotplot", "-f", "paf", "--out-format", "csv", "-l", "4", path)
    assert dev[1] == HEADER + b"100,100,10,15,I,t1,q1\n100,107,10,10,D,t2,q2\n"


def check_error_leaves_nothing(cli, tmp_path):
    """a bad CIGAR op in the last record: the rows of the records in front of it are not written"""
    path = str(tmp_path / "bad.paf")
    with open(path, "wb") as f:
        f.write(b"".join(paf_line("q%d" % k, "t", "5=60I5=") for k in range(6)) + paf_line("q", "t", "10=3"))
    dev, host = both_writers(cli, "dotplot", "-f", "paf", "--out-format", "csv", path, rc=1)
    assert dev[1] == b""
    assert "CIGAR OP `` invalid" in dev[2] and "CIGAR OP `` invalid" in host[2]


def check_gpus(cli, tmp_path, gpus=2):
    """--gpus N: every device writes the rows of its records, the same bytes as one device's"""
    lines = [paf_line("q%d" % (k % 3), "t,%d" % k if k % 4 == 0 else "t%d" % k, "5=%dI3=%dD2=" % (51 + k, 60 + k), ts=1000 * k, neg=k % 2 == 1)
             for k in range(9)]
    path = str(tmp_path / "g.paf")
    with open(path, "wb") as f:
        f.write(b"".join(lines))
    for args in (("dotplot", "-f", "paf", "--out-format", "csv", path), ("dotplot", "--out-format", "csv", "-l", "3", os.path.join(GOLDEN, "test.maf"))):
        one = run(cli, *args)
        many = run(cli, "--gpus", str(gpus), *args)
        assert one[0] == 0 and many[0] == 0, (one[2], many[2])
        assert one[1] == many[1] and one[1].startswith(HEADER) and one[1].count(b"\n") > 3
        assert DEVICE_PHASE in many[2]
        assert run(cli, "--gpus", str(gpus), *args, env=HOST)[1] == one[1]
