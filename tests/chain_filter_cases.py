"""`filter -f chain` on the device (K25): the C-ABI entry (Engine.chain_split -> Engine.chain_filter) against
chain_filter_ref.filter_ref, the restatement that works from the splitter's arrays, and the `wgatools filter -f chain` command
with its device path against its host path and maf_rewrite_ref.filter_chain, the restatement that works from the text.
Imported by test_emu_chain_filter.py (emulator build, CPU) and test_gpu_chain_filter.py (the product on a GPU); each provides
the `cli` and `eng` fixtures."""
import ctypes as C
import gzip

import numpy as np

import chain_filter_ref as ref
import chain_split_cases as cs
import maf_rewrite_ref as mr
import text_items_cases as ti
from wgatools_amd import _lib
from wgatools_amd.engine import CHAIN_FILTER_PARAMS_DTYPE, CHAIN_HEAD_DTYPE, CHAIN_OK

U64 = (1 << 64) - 1
E_INVALID_ARG = -1


# ---- texts ---------------------------------------------------------------------------------------------------------------------
def head(score=b"1000", tname=b"tchr", tsize=100000, tneg=False, ts=10, te=60, qname=b"qchr", qsize=90000, qneg=False, qs=7, qe=57,
         cid=1, sep=b" "):
    """a header line; the numbers may be given as bytes (`+5`, `007`)"""
    f = [b"chain", score, tname, tsize, b"-" if tneg else b"+", ts, te, qname, qsize, b"-" if qneg else b"+", qs, qe, cid]
    return sep.join(x if isinstance(x, bytes) else b"%d" % x for x in f) + b"\n"


def lines(n, k=0):
    """n data lines, the last one the bare `size`"""
    return b"".join(b"%d\t%d\t%d\n" % (5 + (j + k) % 7, (j + k) % 3, (j * 11 + k) % 1234) for j in range(n - 1)) + b"9\n"


def chain(n_lines, k=0, **kw):
    return head(cid=k + 1, **kw) + lines(n_lines, k)


# ---- ABI level -----------------------------------------------------------------------------------------------------------------
class Split:
    """both calls of Engine.chain_split on a file the splitter takes: the device arrays and their host copies"""

    def __init__(self, eng, data):
        self.data = data
        self.d_text = eng.upload(np.frombuffer(data + b"\0" * 16, dtype=np.uint8))
        self.nc, self.nd, st, bad = eng.chain_split(self.d_text, len(data))
        assert (st, bad) == (CHAIN_OK, None), (st, bad, data[:200])
        self.d_heads = eng.empty(self.nc + 1, CHAIN_HEAD_DTYPE)
        self.d_lines = eng.empty((self.nd + 1) * 3, np.uint64)
        self.d_off = eng.empty(self.nc + 1, np.uint64)
        eng.chain_split(self.d_text, len(data), self.d_heads, self.d_lines, self.d_off)
        self.heads = self.d_heads.numpy()[:self.nc]
        self.triples = self.d_lines.numpy()[:3 * self.nd].reshape(self.nd, 3)
        self.off = self.d_off.numpy()

    def args(self):
        return self.d_text, len(self.data), self.d_heads, self.nc, self.d_lines, self.d_off


def check(eng, data, b=0, q=0, sp=None, shift=0):
    """the device's bytes are both restatements' (from the arrays, and from the text)"""
    sp = sp or Split(eng, data)
    text, kept = eng.chain_filter(*sp.args(), b, q, out_shift=shift)         # the guards around d_out are checked in there
    exp, exp_kept = ref.filter_ref(sp.heads, sp.triples, sp.off, data, b, q)
    assert kept == exp_kept and text == exp, (b, q, shift, kept, exp_kept, len(text), len(exp), data[:200])
    assert text == mr.filter_chain(data, b, q), (b, q, data[:200])
    return text


def check_abi_fill_block_edges(eng):
    """256 items per block of the fill: one chain of n data lines is n + 1 items; with a second chain behind it that chain's head
    is item n + 1"""
    for n in (254, 255, 256, 257, 513):
        one = chain(n)
        text = check(eng, one)
        assert text.count(b"\n") == n + 2
        two = one + chain(3, 1, tname=b"second")
        assert check(eng, two).count(b"\n") == n + 2 + 5
        check(eng, two, b=50)
    assert check(eng, chain(255) + chain(3, 1, ts=0, te=10), b=50).count(b"\n") == 257      # the block's last item: a dropped head


def check_abi_stage_limit(eng):
    """600 lines of three times 2^64 - 1: 63 bytes each, 65 with the chain's end — the widest block the stage takes"""
    big = b"%d %d %d\n" % (U64, U64, U64)
    data = head() + big * 600
    text = check(eng, data)
    assert len(text) == len(head()) - 1 + 600 * 63 + 2
    check(eng, chain(2) + data + chain(2, 1))


def check_abi_over_the_stage(eng):
    """heads with names of 9 000 bytes (staged: the block's stretch stays below the stage) and 20 000 bytes (direct)"""
    for n in (9000, 20000):
        for data in (chain(3) + chain(4, 1, tname=b"T" * n) + chain(2, 2) + chain(5, 3, qname=b"Q" * n) + chain(1, 4),
                     chain(2, 0, tname=b"t" * n, qname=b"q" * n),
                     chain(300) + chain(300, 1, tname=b"A" * n, ts=0, te=20) + chain(300, 2, qname=b"B" * n)):
            text = check(eng, data)
            assert len(text) > n
            check(eng, data, b=30)


def check_abi_plan_edges(eng):
    """256 chains per block of the plan pass"""
    for n in (255, 256, 257, 700):
        data = b"".join(chain(1, k, ts=0, te=k % 5) for k in range(n))
        assert check(eng, data).count(b"chain\t") == n
        check(eng, data, b=3)


def check_abi_alignment(eng):
    """target names of 1 .. 33 bytes in successive chains: the heads start at every offset within a 16-byte group; d_out at every
    offset behind an aligned address"""
    data = b"".join(chain(1 + k % 3, k, tname=b"n" * (k + 1)) for k in range(33))
    sp = Split(eng, data)
    text = check(eng, data, sp=sp)
    starts = {i % 16 for i in range(len(text)) if text.startswith(b"chain\t", i)}
    assert starts == set(range(16)), starts
    small = chain(3) + chain(1, 1, tname=b"abcdefg") + chain(40, 2)
    sp2 = Split(eng, small)
    for shift in range(16):
        check(eng, small, sp=sp2, shift=shift)
        check(eng, data, b=51 if shift % 2 else 0, sp=sp, shift=shift)


def check_abi_thresholds(eng):
    spans = (10, 100)
    for name, keep in (("first dropped", [0, 1, 1, 1, 1, 1]), ("last dropped", [1, 1, 1, 1, 1, 0]), ("every other", [1, 0, 1, 0, 1, 0]),
                       ("all dropped", [0] * 6), ("none dropped", [1] * 6)):
        data = b"".join(chain(2 + k, k, ts=5, te=5 + spans[f]) for k, f in enumerate(keep))
        text = check(eng, data, b=50)
        assert text.count(b"chain\t") == sum(keep), name
    sp = Split(eng, data)
    assert eng.chain_filter(*sp.args(), 101, 0) == (b"", 0)                  # nothing kept: 0 bytes, nothing written
    # a dropped chain between two kept ones: inside one block, and across a block's end
    for n in (100, 300):
        data = chain(5, 0, ts=0, te=90) + chain(n, 1, ts=0, te=10) + chain(5, 2, ts=0, te=90)
        assert check(eng, data, b=50).count(b"\n") == 2 * 7
        assert check(eng, data, b=0).count(b"\n") == 2 * 7 + n + 2
    wrap = chain(2, 0, ts=100, te=0)                                         # tend < tstart: the span wraps
    assert check(eng, wrap, b=10 ** 18) == mr.filter_chain(wrap, 0, 0)
    assert check(eng, wrap, b=U64 - 99) == mr.filter_chain(wrap, 0, 0)
    assert check(eng, wrap, b=U64 - 98) == b""
    one = chain(2, 0, qsize=777)
    assert check(eng, one, q=777) == mr.filter_chain(one, 0, 0)              # min_query_size == qsize: kept
    assert check(eng, one, q=778) == b""
    assert check(eng, one, b=50, q=777) != b"" and check(eng, one, b=51, q=777) == b""
    big = head(tsize=U64, ts=0, te=U64, qsize=U64, qs=0, qe=U64, cid=U64 - 1) + lines(1)
    assert check(eng, big, b=U64, q=U64).startswith(b"chain\t1000\ttchr\t%d\t+\t0\t%d\t" % (U64, U64))


def check_abi_values(eng):
    for score, shown in ((b"0", b"0"), (b"007", b"7"), (b"999999999999999", b"999999999999999"), (b"000000000000000", b"0")):
        assert check(eng, head(score=score) + b"5\n").startswith(b"chain\t" + shown + b"\ttchr\t")
    assert check(eng, head(tsize=b"+5", ts=b"+0", te=b"+007", qsize=b"+9", qs=b"+1", qe=b"+2", cid=b"+03") + b"+5 +0 +07\n+5\n") == \
        b"chain\t1000\ttchr\t5\t+\t0\t7\tqchr\t9\t+\t1\t2\t3\n5\t0\t7\n5\t0\t0\n\n"
    assert check(eng, head() + b"5\n5 1\n5 1 2\n").endswith(b"\n5\t0\t0\n5\t1\t0\n5\t1\t2\n\n")      # missing columns print 0
    for tneg in (False, True):
        for qneg in (False, True):
            text = check(eng, chain(2, 0, tneg=tneg, qneg=qneg))
            f = text.split(b"\n")[0].split(b"\t")
            assert (f[4], f[9]) == (b"-" if tneg else b"+", b"-" if qneg else b"+")
    check(eng, head(sep=b" \t ", tname=b"+", qname=b"chain") + b"5  1\t2 \n6\t\n\n\n" + head(sep=b"\x0b", tname=b"12") + b"7\n")


def hand_built(eng, sp, off):
    """the splitter's heads and lines under other offsets"""
    off = np.array(off, dtype=np.uint64)
    assert off[0] == 0 and off[-1] <= sp.nd and len(off) == sp.nc + 1
    d_off = eng.upload(off)
    for b in (0, 50):
        text, kept = eng.chain_filter(sp.d_text, len(sp.data), sp.d_heads, sp.nc, sp.d_lines, d_off, b, 0)
        assert (text, kept) == ref.filter_ref(sp.heads, sp.triples, off, sp.data, b, 0), (off.tolist(), b)
    return eng.chain_filter(sp.d_text, len(sp.data), sp.d_heads, sp.nc, sp.d_lines, d_off)[0]


def check_abi_hand_built(eng):
    """a chain without data lines is legal at this level: its text is the head and the chain's end"""
    data = chain(2, 0) + chain(3, 1, ts=0, te=10) + chain(1, 2) + chain(2, 3, ts=0, te=90)
    sp = Split(eng, data)
    assert sp.off.tolist() == [0, 2, 5, 6, 8]
    text = hand_built(eng, sp, [0, 0, 5, 5, 8])                              # first and a middle one
    assert text.startswith(b"chain\t1000\ttchr\t100000\t+\t10\t60\tqchr\t90000\t+\t7\t57\t1\n\nchain\t")
    text = hand_built(eng, sp, [0, 3, 3, 8, 8])                              # a middle one and the last
    assert text.endswith(b"\t4\n\n")
    assert hand_built(eng, sp, [0, 0, 0, 0, 8]).count(b"\n\n") == 4
    assert hand_built(eng, sp, [0, 8, 8, 8, 8]).count(b"\n\n") == 4
    many = Split(eng, b"".join(chain(1, k) for k in range(600)))            # heads only across the fill's blocks
    off = [0] * 300 + list(range(0, 301))
    assert hand_built(eng, many, off).count(b"chain\t") == 600
    none = eng.upload(np.zeros(1, dtype=np.uint64))
    assert eng.chain_filter(sp.d_text, len(sp.data), sp.d_heads, 0, sp.d_lines, none) == (b"", 0)      # n_chains == 0
    assert eng.chain_filter(None, 0, None, 0, None, None) == (b"", 0)


def raw(eng, sp, d_off=None, work=True, heads=True, nc=None):
    par = np.zeros(1, dtype=CHAIN_FILTER_PARAMS_DTYPE)
    d_work = eng.empty(max(int(eng.lib.wga_chain_filter_work_bytes(sp.nc, sp.nd)), 16), np.uint8)
    total, kept = C.c_uint64(7), C.c_uint64(7)
    rc = eng.lib.wga_chain_filter(eng.ctx, sp.d_text.ptr, len(sp.data), sp.d_heads.ptr if heads else None, sp.nc if nc is None else nc,
                                  sp.d_lines.ptr, (sp.d_off if d_off is None else d_off).ptr, par.ctypes.data, d_work.ptr if work else None,
                                  C.byref(total), C.byref(kept), None)
    return rc


def check_abi_arguments(eng):
    sp = Split(eng, chain(3) + chain(2, 1))
    assert raw(eng, sp) == 0
    assert raw(eng, sp, work=False) == E_INVALID_ARG
    assert raw(eng, sp, work=False, nc=0) == E_INVALID_ARG                  # a null d_work, whatever the counts
    assert raw(eng, sp, heads=False) == E_INVALID_ARG
    assert raw(eng, sp, heads=False, nc=0) == 0
    # n_chains + data lines beyond 0xFFFFFFF0: the call reads the number of lines from the last offset and refuses
    assert raw(eng, sp, d_off=eng.upload(np.array([0, 3, 0xFFFFFFF0 - 1], dtype=np.uint64))) == E_INVALID_ARG
    assert int(eng.lib.wga_chain_filter_work_bytes(0, 0)) >= 8
    assert int(eng.lib.wga_chain_filter_work_bytes(1000, 30000)) == 8 * (1000 + 31000 + 2 + 31000 // 1024 + 4)


def check_abi_count_fill(eng):
    """the fill leaves the counts as the count call set them (Engine.chain_filter checks that); a count call with other
    thresholds on the same workspace does not spoil the pairs of calls behind it"""
    data = b"".join(chain(1 + k % 40, k, ts=0, te=10 * (k % 9)) for k in range(120))
    sp = Split(eng, data)
    work = eng.empty(int(eng.lib.wga_chain_filter_work_bytes(sp.nc, sp.nd)), np.uint8)
    want = {b: ref.filter_ref(sp.heads, sp.triples, sp.off, data, b, 0) for b in (0, 30, 50, 81)}
    for b in (30, 0, 81, 50):
        assert eng.chain_filter_count(*sp.args(), work, b, 0) == (len(want[b][0]), want[b][1])
    assert eng.chain_filter_count(*sp.args(), work, 30, 0) == (len(want[30][0]), want[30][1])
    assert eng.chain_filter_count(*sp.args(), work, 81, 0) == (len(want[81][0]), want[81][1])      # other thresholds in between
    assert eng.chain_filter(*sp.args(), 30, 0, work=work) == want[30]
    assert eng.chain_filter(*sp.args(), 81, 0, work=work) == want[81]
    assert eng.chain_filter(*sp.args(), 0, 0, work=work) == want[0]
    assert want[81] == (b"", 0) and want[0][1] == 120


def item_stream(eng):
    """one chain of 300 data lines and one of 298: 600 items, three blocks of the fill.  The scan of the item sizes stands behind
    the plan in d_work, at word n_chains (capi_chain_write.inc)"""
    data = chain(300) + chain(298, 1, tname=b"second")
    sp = Split(eng, data)
    work = eng.empty(int(eng.lib.wga_chain_filter_work_bytes(sp.nc, sp.nd)), np.uint8)
    total, kept = eng.chain_filter_count(*sp.args(), work)
    want = ref.filter_ref(sp.heads, sp.triples, sp.off, data, 0, 0)[0]
    assert (total, kept) == (len(want), 2)
    par = np.zeros(1, dtype=CHAIN_FILTER_PARAMS_DTYPE)

    def fill(total_bytes, d_out):
        tot, k = C.c_uint64(total_bytes), C.c_uint64(kept)
        assert eng.lib.wga_chain_filter(eng.ctx, sp.d_text.ptr, len(data), sp.d_heads.ptr, sp.nc, sp.d_lines.ptr, sp.d_off.ptr,
                                        par.ctypes.data, work.ptr, C.byref(tot), C.byref(k), d_out) == 0
        assert (tot.value, k.value) == (total_bytes, kept)
    return ti.Stream(eng, work, sp.nc, sp.nc + sp.nd, want, fill)


def check_abi_fill_short_total(eng):
    ti.check_short_total(item_stream(eng))


def check_abi_fill_scan_one_off(eng):
    ti.check_scan_one_off(item_stream(eng), size_checked=False)


def random_file(seed):
    """3 .. 40 chains of 1 .. 400 data lines in the random dress of the accepted grammar"""
    return cs.random_case(100 + seed, 3 + (seed * 37) % 38, 400)


def check_abi_random_files(eng, seeds=range(12)):
    for seed in seeds:
        recs, starts, data = random_file(seed)
        assert 3 <= len(recs) <= 40 and len(data) < 200000
        sp = Split(eng, data)
        sizes = sorted(r["t_ali"] for r in recs)
        for b in (sizes[0], sizes[len(sizes) // 2], sizes[-1]):                # the 0th, 50th and 100th percentile of the sizes
            text = check(eng, data, b, 0, sp)
            assert text == cs.expected_filter(recs, "tchr", 10 ** 8, "qchr", 10 ** 8, starts, b, 0)
        assert check(eng, data, sizes[-1] + 1, 0, sp) == b""


# ---- command level -----------------------------------------------------------------------------------------------------------------
HOST = cs.HOST
run, write = cs.run, cs.write


def path_of(cli, path, env=None):
    rc, out, err = run(cli, "__chain_filter_path", path, env=env)
    assert rc == 0, err
    return out.decode().strip()


PATH_PARTS = 3      # one process per file: the cases are spread over this many tests


def check_path_selection(cli, tmp_path, part):
    """part 0: the random well-formed files under both readers, the accepted files, the empty file; parts 1 and 2: the fallback
    files, half each"""
    if part == 0:
        for seed in (0, 1, 2):
            path = write(tmp_path, "r%d.chain" % seed, random_file(seed)[2])
            assert path_of(cli, path) == "device"
            assert path_of(cli, path, env=HOST) == "host"
        for name, data in cs.ACCEPTED:
            assert path_of(cli, write(tmp_path, name + ".chain", data)) == ("device" if data else "host"), name
        assert path_of(cli, write(tmp_path, "empty.chain", b"")) == "host"
        return
    assert len(cs.FALLBACKS[part - 1::2]) >= 12
    for name, data, bad in cs.FALLBACKS[part - 1::2]:
        assert path_of(cli, write(tmp_path, name + ".chain", data)) == "host", name


def byte_files():
    """name -> (text, a half-kept (-b, -q), whether that pair really keeps some chains and drops some: the chains of
    chain_split_cases.ACCEPTED all have one size, so no pair halves them)"""
    files = {}
    for seed in (0, 1, 2):
        recs, starts, data = random_file(seed)
        sizes = sorted(r["t_ali"] for r in recs)
        files["r%d" % seed] = (data, (sizes[len(sizes) // 2], 0), True)
    for name, data in cs.ACCEPTED:
        files[name] = (data, (20, 5), False)
    files["lines257"] = (chain(257) + chain(3, 1, ts=0, te=10), (50, 0), True)
    files["chains700"] = (b"".join(chain(1, k, ts=0, te=k % 5) for k in range(700)), (3, 0), True)
    files["long_names"] = (chain(3) + chain(4, 1, tname=b"T" * 9000, ts=0, te=10) + chain(2, 2) + chain(5, 3, qname=b"Q" * 20000) +
                           chain(1, 4, ts=0, te=10), (50, 0), True)
    return files


BYTE_FILES = ("r0", "r1", "r2") + tuple(n for n, d in cs.ACCEPTED) + ("lines257", "chains700", "long_names")


def check_bytes(cli, tmp_path, name):
    """device run == host run == the restatement, to stdout, to a file and to a `.gz` file"""
    data, half, halves = byte_files()[name]
    path = write(tmp_path, name + ".chain", data)
    assert path_of(cli, path) == ("device" if data else "host")
    for b, q in ((0, 0), half, (0, U64)):
        want = mr.filter_chain(data, b, q)
        args = ("filter", "-f", "chain", "-b", str(b), "-q", str(q), path)
        assert run(cli, *args) == (0, want, ""), (name, b, q)
        assert run(cli, *args, env=HOST) == (0, want, ""), (name, b, q)
        plain, gz = str(tmp_path / (name + ".out.chain")), str(tmp_path / (name + ".out.chain.gz"))
        assert run(cli, *args, "-o", plain, "-r") == (0, b"", "")
        assert open(plain, "rb").read() == want, (name, b, q)
        assert run(cli, *args, "-o", gz, "-r") == (0, b"", "")
        assert gzip.open(gz, "rb").read() == want, (name, b, q)
    if data:
        want = mr.filter_chain(data, *half)
        assert not halves or (want and want != mr.filter_chain(data, 0, 0)), name      # the pair drops some and keeps some
        assert mr.filter_chain(data, 0, U64) == b""
        assert run(cli, "filter", "-f", "chain", "-b", str(half[0]), "-q", str(half[1]), stdin=data) == (0, want, "")


def check_gpus(cli, tmp_path, gpus=2):
    """the command runs on device 0 whatever --gpus says: the same bytes"""
    data, half, _ = byte_files()["r0"]
    path = write(tmp_path, "g.chain", data)
    args = ("filter", "-f", "chain", "-b", str(half[0]), path)
    one = run(cli, *args)
    assert one[0] == 0 and one[1] == mr.filter_chain(data, half[0], 0)
    assert run(cli, "--gpus", str(gpus), *args) == one


def check_error_order(cli, tmp_path):
    """a file for the host reader with an error: the chains in front of it are written, then the reference's message"""
    front = mr.filter_chain(cs.chain_text(0, 2), 0, 0)
    by_name = {n: d for n, d, _ in cs.FALLBACKS}
    for name, message in (("header_11_tokens", "Parse Chain Error By: Chain Line Field `chain_id` Missing"),
                          ("bad_target_strand", "Parse Strand `*` Error")):
        path = write(tmp_path, name + ".chain", by_name[name])
        assert path_of(cli, path) == "host"
        for env in (None, HOST):
            assert run(cli, "filter", "-f", "chain", path, env=env) == (1, front, message), name
            assert run(cli, "filter", "-f", "chain", "-b", "51", path, env=env) == (1, b"", message), name
