"""`chain2paf` on the device (K27): the C-ABI entry (Engine.chain_split -> Engine.chain2paf) against chain2paf_ref.chain2paf_ref,
the restatement that works from the splitter's arrays, and the `wgatools chain2paf` command with its device path against its
host writer and its host reader.
Imported by test_emu_chain2paf.py (emulator build, CPU) and test_gpu_chain2paf.py (the product on a GPU); each provides the `cli`
and `eng` fixtures."""
import ctypes as C
import gzip
import os
import subprocess

import numpy as np

import chain2paf_ref as ref
import chain_split_cases as cs
import text_items_cases as ti
from chain_filter_cases import Split, chain, head, lines

U64 = (1 << 64) - 1
E_INVALID_ARG = -1


# ---- ABI level -----------------------------------------------------------------------------------------------------------------
def check(eng, data, sp=None, shift=0):
    """the device's bytes and its count are the restatement's; the guards around d_out are checked inside Engine.chain2paf"""
    sp = sp or Split(eng, data)
    text = eng.chain2paf(*sp.args(), out_shift=shift)
    exp = ref.chain2paf_ref(sp.heads, sp.triples, sp.off, data)
    assert text == exp, (shift, len(text), len(exp), data[:200])
    return text


def check_abi_fill_block_edges(eng):
    """256 items per block of the fill: one chain of n data lines is n + 1 items; with a second chain behind it that chain's head
    is item n + 1"""
    for n in (254, 255, 256, 257, 513):
        one = chain(n)
        text = check(eng, one)
        assert text.count(b"\n") == 1 and text.count(b"M") == n
        two = one + chain(3, 1, tname=b"second")
        text = check(eng, two)
        assert text.count(b"\n") == 2 and text.count(b"M") == n + 3


def check_abi_plan_edges(eng):
    """256 chains per block of the plan pass"""
    for n in (255, 256, 257, 700):
        data = b"".join(chain(1, k, ts=0, te=k % 5) for k in range(n))
        assert check(eng, data).count(b"\tcg:Z:9M\n") == n


def check_abi_sums_across_blocks(eng):
    """a chain's sums are differences of scans over all lines: a chain that spans scan blocks (1 024 lines) and fill blocks among
    short ones, sums beyond 2^32, and sums that wrap 2^64"""
    data = chain(3) + chain(2, 1) + chain(600, 2) + chain(1, 3) + chain(1100, 4) + chain(4, 5)
    text = check(eng, data)
    want = sum(5 + (j + 2) % 7 for j in range(599)) + 9
    assert text.split(b"\n")[2].split(b"\t")[9] == b"%d" % want
    big = b"".join(b"%d %d %d\n" % ((1 << 33) - j, (1 << 33) + j, j % 3) for j in range(600))
    text = check(eng, chain(2) + head(cid=7) + big + chain(2, 1))
    f = text.split(b"\n")[1].split(b"\t")
    assert (int(f[9]), int(f[10])) == (sum((1 << 33) - j for j in range(600)), 600 * (1 << 34))
    # the sizes wrap 2^64: 2^63 + 2^63 + 5
    wrap_size = head() + b"%d 1 0\n%d 0 2\n5\n" % (1 << 63, 1 << 63)
    f = check(eng, chain(2) + wrap_size + chain(3, 1)).split(b"\n")[1].split(b"\t")
    assert (f[9], f[10]) == (b"5", b"6")
    # the sizes do not wrap, sizes + 2nd columns do: (2^64 - 10) + 20
    wrap_block = head() + b"%d 7 0\n0 13 1\n3\n" % (U64 - 12)
    f = check(eng, wrap_block + chain(3, 1)).split(b"\n")[0].split(b"\t")
    assert (f[9], f[10]) == (b"%d" % (U64 - 9), b"10")


def check_abi_stage_limit(eng):
    """600 lines of three times 2^64 - 1: 63 bytes each, 64 with the record's end — the widest block the stage takes"""
    big = b"%d %d %d\n" % (U64, U64, U64)
    data = head() + big * 600
    text = check(eng, data)
    assert len(text.split(b"cg:Z:")[1]) == 600 * 63 + 1
    check(eng, chain(2) + data + chain(2, 1))


def check_abi_over_the_stage(eng):
    """heads with names of 9 000 bytes (staged: the block's stretch stays below the stage) and 20 000 bytes (direct): as target,
    as query, and both"""
    for n in (9000, 20000):
        for data in (chain(3) + chain(4, 1, tname=b"T" * n) + chain(2, 2) + chain(5, 3, qname=b"Q" * n) + chain(1, 4),
                     chain(2, 0, tname=b"t" * n, qname=b"q" * n),
                     chain(300) + chain(300, 1, tname=b"A" * n) + chain(300, 2, qname=b"B" * n)):
            assert len(check(eng, data)) > n


def check_abi_values(eng):
    for v in (0, U64):                                                   # every head field
        data = head(score=b"0", tsize=v, ts=v, te=v, qsize=v, qs=v, qe=v, cid=v) + b"5\n"
        want = b"qchr\t%d\t%d\t%d\t+\ttchr\t%d\t%d\t%d\t5\t5\t255\tcg:Z:5M\n" % ((v,) * 6)
        assert check(eng, data) == want
    assert check(eng, head() + b"5 0 3\n5 2 0\n5 0 0\n0 1 1\n0\n").endswith(b"\t15\t18\t255\tcg:Z:5M3I5M2D5M0M1I1D0M\n")
    assert check(eng, head() + b"5\n5 1\n5 1 2\n").endswith(b"\tcg:Z:5M5M1D5M2I1D\n")      # missing columns are zeros
    assert check(eng, head() + b"%d %d %d\n" % (U64, U64, U64)).endswith(b"\tcg:Z:%dM%dI%dD\n" % (U64, U64, U64))
    assert check(eng, head(tsize=b"+5", ts=b"+0", te=b"+007", qsize=b"+9", qs=b"+1", qe=b"+2", cid=b"+03") + b"+5 +0 +07\n+5\n") == \
        b"qchr\t9\t1\t2\t+\ttchr\t5\t0\t7\t10\t10\t255\tcg:Z:5M7I5M\n"
    for tneg in (False, True):                                           # the target's strand does not show
        for qneg in (False, True):
            f = check(eng, chain(2, 0, tneg=tneg, qneg=qneg)).split(b"\t")
            assert f[4] == (b"-" if qneg else b"+") and len(f) == 13
            assert check(eng, chain(2, 0, tneg=tneg, qneg=qneg)) == check(eng, chain(2, 0, qneg=qneg))
    # a deletion counts once on either strand
    assert check(eng, head(qneg=True) + b"5 4 1\n3\n").endswith(b"\t-\ttchr\t100000\t10\t60\t8\t12\t255\tcg:Z:5M1I4D3M\n")


QUOTED = (b'"', b'a"b', b'""x""', b"n" * 299 + b'"', b'"' + b"q" * 19998 + b'"')


def check_abi_quoting(eng):
    """a name with a quote goes between quotes, the quotes inside doubled: as query, as target, and both; the count is the
    restatement's length (Engine.chain2paf allocates by it and checks the guards)"""
    for name in QUOTED:
        q = b'"' + name.replace(b'"', b'""') + b'"'
        plain = check(eng, chain(2))
        as_q = check(eng, chain(3) + chain(2, 0, qname=name) + chain(1, 1))
        assert as_q.split(b"\n")[1] == plain.replace(b"qchr", q)[:-1]
        as_t = check(eng, chain(2, 0, tname=name) + chain(300, 1))
        assert as_t.split(b"\n")[0] == plain.replace(b"tchr", q)[:-1]
        both = check(eng, chain(2, 0, tname=name, qname=name))
        assert both == plain.replace(b"qchr", q).replace(b"tchr", q)
    check(eng, b"".join(chain(1 + k % 3, k, tname=QUOTED[k % 4], qname=QUOTED[(k + 1) % 4]) for k in range(300)))


def hand_built(eng, sp, off):
    """the splitter's heads and lines under other offsets"""
    off = np.array(off, dtype=np.uint64)
    assert off[0] == 0 and off[-1] <= sp.nd and len(off) == sp.nc + 1
    text = eng.chain2paf(sp.d_text, len(sp.data), sp.d_heads, sp.nc, sp.d_lines, eng.upload(off))
    assert text == ref.chain2paf_ref(sp.heads, sp.triples, off, sp.data), off.tolist()
    return text


def check_abi_hand_built(eng):
    """a chain without data lines is legal at this level: its record ends in `cg:Z:` and the newline, its sums are 0"""
    data = chain(2, 0) + chain(3, 1) + chain(1, 2) + chain(2, 3)
    sp = Split(eng, data)
    assert sp.off.tolist() == [0, 2, 5, 6, 8]
    text = hand_built(eng, sp, [0, 0, 5, 5, 8])                              # first and a middle one
    assert text.startswith(b"qchr\t90000\t7\t57\t+\ttchr\t100000\t10\t60\t0\t0\t255\tcg:Z:\nqchr\t")
    assert text.count(b"\tcg:Z:\n") == 2
    text = hand_built(eng, sp, [0, 3, 3, 8, 8])                              # a middle one and the last
    assert text.endswith(b"\t0\t0\t255\tcg:Z:\n") and text.count(b"\tcg:Z:\n") == 2
    assert hand_built(eng, sp, [0, 0, 0, 0, 8]).count(b"\n") == 4
    assert hand_built(eng, sp, [0, 8, 8, 8, 8]).count(b"\n") == 4
    many = Split(eng, b"".join(chain(1, k) for k in range(600)))            # heads only across the fill's blocks
    assert hand_built(eng, many, [0] * 300 + list(range(0, 301))).count(b"\n") == 600
    none = eng.upload(np.zeros(1, dtype=np.uint64))
    assert eng.chain2paf(sp.d_text, len(sp.data), sp.d_heads, 0, sp.d_lines, none) == b""      # n_chains == 0
    assert eng.chain2paf(None, 0, None, 0, None, None) == b""


def check_abi_alignment(eng):
    """records of one odd length, one after the other: they start at every offset within a 16-byte group; d_out at every offset
    behind an aligned address"""
    one = check(eng, chain(1))
    pad = b"n" * (1 + len(one) % 2)
    data = b"".join(chain(1, k, qname=b"qchr" + pad) for k in range(20)) + b"".join(chain(1 + k % 3, k, tname=b"t" * (k + 1)) for k in range(9))
    sp = Split(eng, data)
    text = check(eng, data, sp=sp)
    starts, at = set(), 0
    for rec in text.split(b"\n")[:-1]:
        starts.add(at % 16)
        at += len(rec) + 1
    assert starts == set(range(16)), starts
    small = chain(3) + chain(1, 1, tname=b'abc"defg') + chain(40, 2)
    sp2 = Split(eng, small)
    for shift in range(16):
        check(eng, small, sp=sp2, shift=shift)
        check(eng, data, sp=sp, shift=shift)


def check_abi_count_fill(eng):
    """*total_bytes is the restatement's length, also from a workspace that other arrays' calls used before"""
    work = eng.empty(int(eng.lib.wga_chain2paf_work_bytes(130, 3000)), np.uint8)
    for seed in (0, 1):
        data = b"".join(chain(1 + (k + seed) % 40, k, qname=b"q%d" % k) for k in range(120 + seed))
        sp = Split(eng, data)
        want = ref.chain2paf_ref(sp.heads, sp.triples, sp.off, data)
        assert eng.chain2paf_count(*sp.args(), work) == len(want)
        assert eng.chain2paf(*sp.args(), work=work) == want


def raw(eng, sp, d_off=None, work=True, heads=True, text=True, off=True, nc=None):
    d_work = eng.empty(max(int(eng.lib.wga_chain2paf_work_bytes(sp.nc, sp.nd)), 16), np.uint8)
    total = C.c_uint64(7)
    d_off = (sp.d_off if d_off is None else d_off).ptr if off else None
    return eng.lib.wga_chain2paf(eng.ctx, sp.d_text.ptr if text else None, len(sp.data), sp.d_heads.ptr if heads else None,
                                 sp.nc if nc is None else nc, sp.d_lines.ptr, d_off, d_work.ptr if work else None, C.byref(total), None)


def check_abi_arguments(eng):
    sp = Split(eng, chain(3) + chain(2, 1))
    assert raw(eng, sp) == 0
    assert raw(eng, sp, work=False) == E_INVALID_ARG
    assert raw(eng, sp, work=False, nc=0) == E_INVALID_ARG                  # a null d_work, whatever the counts
    for null in ("heads", "text", "off"):
        assert raw(eng, sp, **{null: False}) == E_INVALID_ARG
        assert raw(eng, sp, nc=0, **{null: False}) == 0
    # n_chains + data lines beyond 0xFFFFFFF0: the call reads the number of lines from the last offset and refuses (counts only)
    assert raw(eng, sp, d_off=eng.upload(np.array([0, 3, 0xFFFFFFF0 - 1], dtype=np.uint64))) == E_INVALID_ARG
    assert raw(eng, sp, d_off=eng.upload(np.array([0, 3, U64], dtype=np.uint64))) == E_INVALID_ARG
    assert int(eng.lib.wga_chain2paf_work_bytes(0, 0)) >= 8
    assert int(eng.lib.wga_chain2paf_work_bytes(1000, 30000)) == 8 * (3 * 1000 + 31000 + 1 + 2 * 30001 + 31000 // 1024 + 4)


def item_stream(eng):
    """one chain of 300 data lines and one of 298: 600 items, three blocks of the fill.  The scan of the item sizes stands behind
    the plan and the sums in d_work, at word 3 n_chains (capi_chain2paf.inc)"""
    data = chain(300) + chain(298, 1, tname=b"second")
    sp = Split(eng, data)
    work = eng.empty(int(eng.lib.wga_chain2paf_work_bytes(sp.nc, sp.nd)), np.uint8)
    want = ref.chain2paf_ref(sp.heads, sp.triples, sp.off, data)
    assert eng.chain2paf_count(*sp.args(), work) == len(want)

    def fill(total_bytes, d_out):
        tot = C.c_uint64(total_bytes)
        assert eng.lib.wga_chain2paf(eng.ctx, sp.d_text.ptr, len(data), sp.d_heads.ptr, sp.nc, sp.d_lines.ptr, sp.d_off.ptr, work.ptr,
                                     C.byref(tot), d_out) == 0
        assert tot.value == total_bytes
    return ti.Stream(eng, work, 3 * sp.nc, sp.nc + sp.nd, want, fill)


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
        assert check(eng, data) == cs.expected_chain2paf(recs, "tchr", 10 ** 8, "qchr", 10 ** 8, starts)


# ---- command level -----------------------------------------------------------------------------------------------------------------
HOST_READER = cs.HOST
HOST_WRITER = {"WGA_CHAIN2PAF_WRITER": "host"}
run, write = cs.run, cs.write


def path_of(cli, path, env=None, gpus=None):
    rc, out, err = run(cli, *(("--gpus", str(gpus)) if gpus else ()), "__chain2paf_path", path, env=env)
    assert rc == 0, err
    return out.decode().strip()


def quoted_file():
    return (chain(3, 0, qname=b'a"b') + chain(300, 1, tname=b'"') + chain(2, 2, tname=b'""x""', qname=b"n" * 299 + b'"') +
            chain(5, 3, qname=QUOTED[4]) + chain(1, 4))


def byte_files():
    """name -> (text, the path the command takes for it, the expected bytes or None)"""
    files = {}
    for seed in (0, 1, 2):
        recs, starts, data = random_file(seed)
        files["r%d" % seed] = (data, "device", cs.expected_chain2paf(recs, "tchr", 10 ** 8, "qchr", 10 ** 8, starts))
    files["quoted"] = (quoted_file(), "device", None)
    files["empty"] = (b"", "host", b"")
    by_name = {n: d for n, d, _ in cs.FALLBACKS}
    for name in ("cr", "comment_between"):
        files[name] = (by_name[name], "host", None)
    files["score_1e3"] = (cs.chain_text(0, 2) + cs.head_line(1, score=b"1e3") + b"5\n", "host", None)
    return files


BYTE_FILES = ("r0", "r1", "r2", "quoted", "empty", "cr", "comment_between", "score_1e3")


def check_bytes(cli, tmp_path, name):
    """the device path, the host writer and the host reader: the same bytes, exit status and message; a `.gz` holds them too"""
    data, path_want, want = byte_files()[name]
    path = write(tmp_path, name + ".chain", data)
    assert path_of(cli, path) == path_want
    got = run(cli, "chain2paf", path)
    assert got[0] in (0, 1)
    assert run(cli, "chain2paf", path, env=HOST_WRITER) == got, name
    assert run(cli, "chain2paf", path, env=HOST_READER) == got, name
    if want is not None:
        assert got == (0, want, ""), name
    if name == "quoted":
        assert got[0] == 0 and got[1].count(b'"a""b"\t') == 1 and got[1].count(b'\t""""\t') == 1 and got[1].count(b"\n") == 5
    if path_want == "device":
        gz = str(tmp_path / (name + ".paf.gz"))
        assert run(cli, "chain2paf", path, "-o", gz, "-r") == (0, b"", "")
        assert gzip.open(gz, "rb").read() == got[1], name
        assert run(cli, "chain2paf", stdin=data) == got


def check_path_selection(cli, tmp_path):
    """`device` for a plain file; `host` under either switch"""
    path = write(tmp_path, "p.chain", random_file(3)[2])
    assert path_of(cli, path) == "device"
    assert path_of(cli, path, env=HOST_WRITER) == "host"
    assert path_of(cli, path, env=HOST_READER) == "host"
    assert path_of(cli, path, env={"WGA_CHAIN2PAF_WRITER": "device"}) == "device"


def check_wide_values(cli, tmp_path):
    """data lines that need more packed ops than three per line keep the host writer, whatever it does with them: a value of 2^28
    is two ops (the same bytes from all three ways), 2^64 - 1 is 2^36 of them (the same outcome from all three ways)"""
    one_op = write(tmp_path, "w0.chain", head() + b"%d 1 1\n" % ((1 << 28) - 1))
    assert path_of(cli, one_op) == "device"
    assert run(cli, "chain2paf", one_op) == (0, b"qchr\t90000\t7\t57\t+\ttchr\t100000\t10\t60\t268435455\t268435456\t255\tcg:Z:268435455M1I1D\n", "")
    two_ops = write(tmp_path, "w1.chain", head() + b"%d 1 1\n" % (1 << 28))
    assert path_of(cli, two_ops) == "host"
    got = run(cli, "chain2paf", two_ops)
    assert got == (0, b"qchr\t90000\t7\t57\t+\ttchr\t100000\t10\t60\t268435456\t268435457\t255\tcg:Z:268435456M1I1D\n", "")
    widest = write(tmp_path, "w2.chain", head() + b"%d %d %d\n1\n" % (U64, U64, U64))
    assert path_of(cli, widest) == "host"
    for path in (two_ops, widest):
        got = run(cli, "chain2paf", path)
        assert got[0] in (0, 1)
        assert run(cli, "chain2paf", path, env=HOST_WRITER) == got and run(cli, "chain2paf", path, env=HOST_READER) == got


def check_timing_phase(cli, tmp_path):
    """WGA_TIMING=1 names the phase after the writer that ran"""
    path = write(tmp_path, "t.chain", random_file(4)[2])
    for env, phase in (({}, "chain2paf records (device)"), (HOST_WRITER, "chain2paf records (host)")):
        r = subprocess.run([cli, "chain2paf", path], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                           env=dict(os.environ, WGA_TIMING="1", **env))
        assert r.returncode == 0 and phase in r.stderr.decode(errors="replace"), r.stderr[-2000:]


def check_gpus(cli, tmp_path, gpus=2):
    """--gpus N keeps the host writer over N devices: `host`, and the bytes of the device path"""
    recs, starts, data = random_file(5)
    path = write(tmp_path, "g.chain", data)
    one = run(cli, "chain2paf", path)
    assert one == (0, cs.expected_chain2paf(recs, "tchr", 10 ** 8, "qchr", 10 ** 8, starts), "")
    assert path_of(cli, path, gpus=gpus) == "host"
    assert run(cli, "--gpus", str(gpus), "chain2paf", path) == one
