"""Chain reader cases: the C-ABI entry (Engine.chain_split, K23) against a plain-Python restatement of the rules of the plain
chain file (include/wga_hip.h, wga_chain_split), and the `wgatools` chain commands with the device reader against the host
reader and the oracle.  Imported by test_emu_chain_split.py (emulator build, CPU) and test_gpu_chain_split.py (the product on a
GPU); each provides the `cli` and `eng` fixtures."""
import os
import random
import re
import subprocess

import numpy as np

import oracle_py as orc
from wgatools_amd.engine import CHAIN_FALLBACK, CHAIN_HEAD_DTYPE, CHAIN_OK

U64 = (1 << 64) - 1
BLANK, HEADER, DATA = 0, 1, 2
_WS = re.compile(rb"[\t\x0b\x0c\r ]+")          # the ASCII white space of split_whitespace, the newline aside
_U64 = re.compile(rb"\+?[0-9]{1,20}")
_SCORE = re.compile(rb"[0-9]{1,15}")


# ---- the restatement -----------------------------------------------------------------------------------------------------
def _kind(line):
    if not line:
        return BLANK
    if len(line) >= 6 and line[:5] == b"chain" and line[5:6] in (b"\t", b"\x0b", b"\x0c", b"\r", b" "):
        return HEADER
    return DATA


def _u64(tok):
    if not _U64.fullmatch(tok) or int(tok) > U64:
        return None
    return int(tok)


def _header(tok):
    """the 13 leading tokens of a header line -> (score, tname, tsize, tneg, tstart, tend, qname, qsize, qneg, qstart, qend, id)"""
    if len(tok) < 13 or not _SCORE.fullmatch(tok[1]) or tok[4] not in (b"+", b"-") or tok[9] not in (b"+", b"-"):
        return None
    nums = [_u64(tok[k]) for k in (3, 5, 6, 8, 10, 11, 12)]
    if None in nums:
        return None
    return (int(tok[1]), tok[2], nums[0], tok[4] == b"-", nums[1], nums[2], tok[7], nums[3], tok[9] == b"-", nums[4], nums[5], nums[6])


def split_ref(data):
    """(status, first bad line or None, heads, triples, line_off): which files the device takes, and what it yields for them"""
    if not data:
        return CHAIN_OK, None, [], [], [0]
    lines = data.split(b"\n")
    terminated = lines[-1] == b""
    if terminated:
        lines.pop()
    kinds = [_kind(ln) for ln in lines]
    heads, triples, line_off, bad = [], [], [], None
    for j, (ln, k) in enumerate(zip(lines, kinds)):
        ok = terminated or j + 1 < len(lines)                        # the last line ends in a newline
        ok = ok and b"\r" not in ln and max(ln, default=0) < 0x80
        if j == 0:
            ok = ok and k == HEADER                                  # the first line is a header
        elif k == DATA:
            ok = ok and kinds[j - 1] != BLANK                        # a data line follows a header or a data line
        else:
            ok = ok and kinds[j - 1] != HEADER                       # a header is followed by a data line
        tok = [t for t in _WS.split(ln) if t]
        if k == HEADER:
            ok = ok and j + 1 < len(lines)                           # ... also at the end of the file
            h = _header(tok)
            ok = ok and h is not None
            heads.append(h)
            line_off.append(len(triples))
        elif k == DATA:
            v = [_u64(t) for t in tok]
            ok = ok and 1 <= len(v) <= 3 and None not in v
            triples.append(tuple((v + [0, 0, 0])[:3]) if ok else None)
        if not ok and bad is None:
            bad = j
    line_off.append(len(triples))
    return (CHAIN_OK if bad is None else CHAIN_FALLBACK), bad, heads, triples, line_off


# ---- ABI level -------------------------------------------------------------------------------------------------------------
GUARD = 0xA5


def abi(eng, data):
    """both calls of Engine.chain_split: (status, bad, heads, triples, line_off, d_lines, d_line_off), guards checked"""
    d_text = eng.upload(np.frombuffer(data + b"\0" * 16, dtype=np.uint8))
    nc, nd, st, bad = eng.chain_split(d_text, len(data))
    d_heads = eng.empty(nc + 1, CHAIN_HEAD_DTYPE).fill(GUARD)
    d_lines = eng.empty((nd + 1) * 3, np.uint64).fill(GUARD)
    d_off = eng.empty(nc + 2, np.uint64).fill(GUARD)
    assert eng.chain_split(d_text, len(data), d_heads, d_lines, d_off) == (nc, nd, st, bad)
    heads, lines, off = d_heads.numpy(), d_lines.numpy(), d_off.numpy()
    assert heads[nc:].tobytes() == bytes([GUARD]) * CHAIN_HEAD_DTYPE.itemsize
    assert (lines[3 * nd:] == int.from_bytes(bytes([GUARD]) * 8, "little")).all()
    assert off[nc + 1] == int.from_bytes(bytes([GUARD]) * 8, "little")
    return st, bad, heads[:nc], lines[:3 * nd].reshape(nd, 3), off[:nc + 1], d_lines, d_off


def check(eng, data, status=None, bad=None):
    """the device's answer == the restatement's; status / bad: what the case itself expects of both"""
    exp = split_ref(data)
    got = abi(eng, data)
    assert (got[0], got[1]) == (exp[0], exp[1]), (got[:2], exp[:2], data[:200])
    if status is not None:
        assert (exp[0], exp[1]) == (status, bad), (exp[:2], status, bad, data[:200])
    assert len(got[2]) == len(exp[2]) and len(got[3]) == len(exp[3])        # the counts hold for a fallback file too
    if exp[0] != CHAIN_OK:
        return got
    assert got[4].tolist() == exp[4]
    assert got[3].tolist() == [list(t) for t in exp[3]]
    for h, e in zip(got[2], exp[2]):
        assert h["num"].tolist() == [e[0], e[2], e[4], e[5], e[7], e[9], e[10], e[11]], e
        assert (bool(h["tstrand_neg"]), bool(h["qstrand_neg"])) == (e[3], e[8])
        assert data[int(h["tname_off"]):int(h["tname_off"]) + int(h["tname_len"])] == e[1]
        assert data[int(h["qname_off"]):int(h["qname_off"]) + int(h["qname_len"])] == e[6]
        assert h["pad"].tolist() == [0] * 6
    return got


def head_line(k=0, tname=b"tchr", qname=b"qchr", score=b"1000", sep=b" ", extra=b"", qneg=False):
    f = [b"chain", score, tname, b"100000", b"+", b"%d" % (10 * k), b"%d" % (10 * k + 50), qname, b"90000",
         b"-" if qneg else b"+", b"%d" % (7 * k), b"%d" % (7 * k + 50), b"%d" % (k + 1)]
    return sep.join(f) + extra + b"\n"


def chain_text(k, n_lines, **kw):
    """a chain of n_lines data lines, the last one the bare `size`"""
    return head_line(k, **kw) + b"".join(b"%d\t%d\t%d\n" % (5 + j % 7, j % 3, (j + 1) % 4) for j in range(n_lines - 1)) + b"9\n"


def check_abi_tile_and_block_edges(eng):
    """the delimiter pass works on 4 KiB of text per block, the line passes on 256 lines per block"""
    for edge in (4096, 8192):
        lead = b"".join(chain_text(k, 40) for k in range(64))
        for shift in range(0, 70, 3):                                  # the header line straddles the edge byte by byte
            pre = lead[:lead.rindex(b"\nchain", 0, edge - shift) + 1]
            pad = edge - shift - len(pre)                                # blank lines in front of the header bring it there
            if pad < 0:
                continue
            data = pre + b"\n" * pad + chain_text(99, 3, tname=b"chrStraddle_0123456789", qname=b"q" * 30) + chain_text(100, 2)
            assert data[edge - shift:edge - shift + 6] == b"chain "
            check(eng, data, CHAIN_OK)
    for at in (4095, 4096):                                            # a newline exactly there
        one = chain_text(0, 5)
        fill = at + 1 - len(one) - len(head_line(1))
        data = one + head_line(1) + b"".join(b"7\t1\t1\n" for _ in range(fill // 6 - 1))
        data += b"1" * (at - len(data)) + b"\n" + b"3\n"
        assert data[at:at + 1] == b"\n" and data[at - 1:at] != b"\n"
        check(eng, data, CHAIN_OK)
    for n in (255, 256, 257):
        check(eng, chain_text(0, n - 1), CHAIN_OK)                      # exactly n lines
        assert chain_text(0, n - 1).count(b"\n") == n
        got = check(eng, b"".join(chain_text(k, 1) for k in range(n)), CHAIN_OK)      # exactly n chains, a bare `size` each
        assert len(got[2]) == n
        got = check(eng, b"".join(chain_text(k, 2) + b"\n" for k in range(n)), CHAIN_OK)
        assert len(got[2]) == n
    got = check(eng, chain_text(0, 1) + chain_text(1, 700) + chain_text(2, 1), CHAIN_OK)      # 700 data lines: three line blocks
    assert got[4].tolist() == [0, 1, 701, 702]


TOKEN_FILES = []      # every text check_abi_tokens looks at: the command-level cases run them through both readers


def check_abi_tokens(eng, collect=None):
    def check_(e, data, *a):
        if collect is not None:
            collect.append(data)
            return abi_like_ref(data)
        return check(e, data, *a)
    ok = lambda d: check_(eng, d, CHAIN_OK)
    ok(head_line(0, sep=b"\t") + b"5\t1\t2\n6\n")
    ok(head_line(0, sep=b"   ") + b"5  1   2\n6\n")
    ok(head_line(0, sep=b"\x0b") + b"5\x0b1\x0c2\n6\n")
    ok(head_line(0, sep=b" \t\x0c") + b"5\t \t1 2\n6\n")
    ok(head_line(0, extra=b" \t ") + b"5 1 2 \t\n6\t\n")                   # trailing white space
    ok(head_line(0) + b"+7 +0 +3\n+7\n")
    got = ok(head_line(0) + b"18446744073709551615 18446744073709551615 18446744073709551615\n1\n")
    assert got[3][0].tolist() == [U64] * 3
    check_(eng, head_line(0) + b"18446744073709551616\n1\n", CHAIN_FALLBACK, 1)
    check_(eng, head_line(0) + b"5 18446744073709551616\n1\n", CHAIN_FALLBACK, 1)
    got = ok(head_line(0) + b"5\n5 1\n5 1 2\n")                            # 1, 2 and 3 numbers
    assert got[3].tolist() == [[5, 0, 0], [5, 1, 0], [5, 1, 2]]
    ok(head_line(0, extra=b" surplus") + b"5\n")                             # 13 and 14 tokens behind "chain"
    ok(head_line(0, extra=b" surplus 1e3") + b"5\n")
    ok(head_line(0, score=b"0") + b"5\n")
    got = ok(head_line(0, score=b"999999999999999") + b"5\n")
    assert int(got[2][0]["num"][0]) == 999999999999999
    for score in (b"1000000000000000", b"1e3", b"1.5", b"+1", b"nan"):
        check_(eng, chain_text(0, 2) + head_line(1, score=score) + b"5\n", CHAIN_FALLBACK, 3)
    ok(head_line(0, tname=b"c", qname=b"chain") + b"5\n" + head_line(1, tname=b"chain1", qname=b"7c7") + b"5\n")
    ok(head_line(0, tname=b"12", qname=b"scaffold_chain_c") + b"5\n")
    got = ok(head_line(0, tname=b"+", qname=b"-", qneg=True) + b"5\n")
    assert bool(got[2][0]["qstrand_neg"]) and not bool(got[2][0]["tstrand_neg"])
    for k in (3, 5, 6, 8, 10, 11, 12):                                    # the eight integers like u64::from_str
        f = head_line(0).split(b" ")
        f[k] = b"+" + f[k].strip()
        ok(b" ".join(f) + (b"\n" if k == 12 else b"") + b"5\n")
        f[k] = b"18446744073709551616"
        check_(eng, b" ".join(f) + (b"\n" if k == 12 else b"") + b"5\n", CHAIN_FALLBACK, 0)
        f[k] = b"-1"
        check_(eng, b" ".join(f) + (b"\n" if k == 12 else b"") + b"5\n", CHAIN_FALLBACK, 0)


def abi_like_ref(data):
    """the restatement's answer in the shape of abi()'s (collecting the token files needs no engine)"""
    st, bad, heads, triples, off = split_ref(data)
    h = np.zeros(len(heads), dtype=CHAIN_HEAD_DTYPE)
    for k, e in enumerate(heads):
        if e is not None:
            h[k]["num"] = [e[0], e[2], e[4], e[5], e[7], e[9], e[10], e[11]]
            h[k]["tstrand_neg"], h[k]["qstrand_neg"] = e[3], e[8]
    t = np.array([x if x is not None else (0, 0, 0) for x in triples], dtype=np.uint64).reshape(len(triples), 3)
    return st, bad, h, t, np.array(off, dtype=np.uint64), None, None


check_abi_tokens(None, TOKEN_FILES)


# one file per rule that falls back: (name, text, first offending line)
GOOD2 = chain_text(0, 3) + b"\n" + chain_text(1, 2) + b"\n"              # lines 0 .. 7
FALLBACKS = [
    ("cr", chain_text(0, 3) + b"\n" + head_line(1) + b"5\r\n6\n", 6),
    ("cr_in_header", chain_text(0, 2) + head_line(1, extra=b"\r") + b"5\n", 3),
    ("high_byte_in_name", chain_text(0, 2) + head_line(1, tname="chré".encode()) + b"5\n", 3),
    ("no_trailing_newline", chain_text(0, 3) + b"\n" + head_line(1) + b"5\t1\t1\n6", 7),
    ("white_space_only_line", chain_text(0, 2) + b" \t \n" + chain_text(1, 2), 3),
    ("chain1", chain_text(0, 2) + b"chain1 t 100 + 0 13 q 100 + 0 14 1\n5\n", 3),
    ("leading_space", chain_text(0, 2) + b" " + head_line(1) + b"5\n", 3),
    ("header_11_tokens", chain_text(0, 2) + b"chain 1 t 100 + 0 13 q 100 + 0 14\n5\n", 3),
    ("bad_target_strand", chain_text(0, 2) + b"chain 1 t 100 * 0 13 q 100 + 0 14 1\n5\n", 3),
    ("bad_query_strand", chain_text(0, 2) + b"chain 1 t 100 + 0 13 q 100 ++ 0 14 1\n5\n", 3),
    ("data_4_tokens", head_line(0) + b"5 1 2\n5 1 2 3\n6\n", 2),
    ("letter_in_data", head_line(0) + b"5 1 2\n5 x 2\n6\n", 2),
    ("letter_glued_to_digits", head_line(0) + b"5 1 2\n5 1 2x\n6\n", 2),
    ("minus_one", head_line(0) + b"5 -1 2\n6\n", 1),
    ("header_then_header", chain_text(0, 2) + head_line(1) + head_line(2) + b"5\n", 4),
    ("header_then_blank", chain_text(0, 2) + head_line(1) + b"\n5\n", 4),
    ("header_at_eof", chain_text(0, 2) + b"\n" + head_line(1), 4),
    ("data_after_blank", chain_text(0, 2) + b"\n7\n" + chain_text(1, 2), 4),
    ("comment_first", b"#comment\n" + GOOD2, 0),
    ("track_first", b"track name=x and more\n" + GOOD2, 0),
    ("blank_first", b"\n" + GOOD2, 0),
    ("comment_between", chain_text(0, 2) + b"\n#comment\n" + chain_text(1, 2), 4),
    ("comment_behind_data", chain_text(0, 2) + b"# comment\n" + chain_text(1, 2), 3),
    ("bare_chain", chain_text(0, 2) + b"chain\n5\n", 3),
    ("only_a_newline", b"\n", 0),
]
ACCEPTED = [
    ("header_directly_after_data", chain_text(0, 3) + chain_text(1, 2) + chain_text(2, 1)),
    ("three_blank_lines_between", chain_text(0, 3) + b"\n\n\n" + chain_text(1, 2) + b"\n\n\n"),
    ("empty_file", b""),
]


def check_abi_order_rules(eng):
    for name, data, bad in FALLBACKS:
        check(eng, data, CHAIN_FALLBACK, bad)
    for name, data in ACCEPTED:
        got = check(eng, data, CHAIN_OK)
    assert abi(eng, b"")[4].tolist() == [0]
    check(eng, GOOD2, CHAIN_OK)
    two_bad = chain_text(0, 2) + b"x\n" + chain_text(1, 300) + b"y\n"        # the smallest index wins across line blocks
    check(eng, two_bad, CHAIN_FALLBACK, 3)


# ---- random well-formed files (the accepted grammar only) -----------------------------------------------------------------
def synth_chain(seed, n, max_lines=120):
    """cli_cases._synth_chain's records: consistent lengths, so that the converters take them"""
    rng = np.random.default_rng(seed)
    recs = []
    for k in range(n):
        nl = int(rng.integers(1, max_lines + 1))
        lines = [(int(rng.integers(1, 60)), int(rng.integers(0, 3)) * int(rng.integers(0, 12)),
                  int(rng.integers(0, 3)) * int(rng.integers(0, 12))) for _ in range(nl)]
        lines[-1] = (lines[-1][0], 0, 0)
        recs.append(dict(lines=lines, t_ali=sum(s + dt for s, dt, dq in lines), q_ali=sum(s + dq for s, dt, dq in lines),
                         neg=bool(rng.integers(0, 2)), id=int(rng.integers(0, 10 ** 6))))
    return recs


def random_text(recs, t_name, t_size, q_name, q_size, starts, seed):
    """the records in a random dress of the accepted grammar: separators, '+', trailing white space, surplus header tokens,
    short last lines, blank lines behind a chain or none"""
    rng = random.Random(seed)
    sep = lambda: rng.choice([b" ", b"\t", b"  ", b" \t", b"\x0b", b"\x0c "])
    num = lambda v: (b"+" if rng.random() < 0.1 else b"") + b"%d" % v
    out = []
    for r, (ts, qs) in zip(recs, starts):
        f = [b"chain", b"%d" % (1000 + r["id"]), t_name, num(t_size), b"+", num(ts), num(ts + r["t_ali"]), q_name, num(q_size),
             b"-" if r["neg"] else b"+", num(qs), num(qs + r["q_ali"]), num(r["id"])]
        if rng.random() < 0.2:
            f.append(rng.choice([b"extra", b"1e3 chain", b"c"]))
        out.append(b"".join(x + sep() for x in f[:-1]) + f[-1] + (sep() if rng.random() < 0.2 else b"") + b"\n")
        for j, (s, dt, dq) in enumerate(r["lines"]):
            last = j == len(r["lines"]) - 1
            cols = [s] if last and rng.random() < 0.7 else [s, dt] if dq == 0 and rng.random() < 0.2 else [s, dt, dq]
            out.append(b"".join(num(c) + sep() for c in cols[:-1]) + num(cols[-1]) + (sep() if rng.random() < 0.1 else b"") + b"\n")
        out.append(b"\n" * rng.choice([0, 1, 1, 1, 3]))
    return b"".join(out)


def random_case(seed=11, n=200, max_lines=120, T=10 ** 8, Q=10 ** 8):
    recs = synth_chain(seed, n, max_lines)
    rng = np.random.default_rng(seed + 1)
    starts = [(int(rng.integers(0, T - r["t_ali"] - 1)), int(rng.integers(0, Q - r["q_ali"] - 1))) for r in recs]
    return recs, starts, random_text(recs, b"tchr", T, b"qchr", Q, starts, seed + 2)


def check_abi_random_files(eng):
    """200 chains of up to 120 lines: taken, and the device arrays go straight into wga_chain_lines_ops"""
    recs, starts, data = random_case()
    assert len(data) < 250000
    st, bad, heads, lines, off, d_lines, d_off = check(eng, data, CHAIN_OK)
    assert [r["lines"] for r in recs] == [[tuple(t) for t in lines[int(off[k]):int(off[k + 1])].tolist()] for k in range(len(recs))]
    assert [(int(h["num"][7]), bool(h["qstrand_neg"])) for h in heads] == [(r["id"], r["neg"]) for r in recs]
    n, ne = len(recs), len(lines)

    def ops_of(dl, do):
        cnt = eng.chain_lines_ops(n, ne, dl, do)
        ooff = eng.exclusive_scan_u64(n, cnt)
        ops = eng.empty(int(ooff.numpy()[-1]) + 4, np.uint32).fill(0xFF)
        eng.chain_lines_ops(n, ne, dl, do, out=ops, out_off=ooff)
        return ooff.numpy().tolist(), ops.numpy().tolist()
    flat = np.array([v for r in recs for ln in r["lines"] for v in ln] + [0, 0, 0], dtype=np.uint64)
    host_off = np.cumsum([0] + [len(r["lines"]) for r in recs]).astype(np.uint64)
    assert ops_of(d_lines, d_off) == ops_of(eng.upload(flat), eng.upload(host_off))
    for seed in range(20, 26):                                          # more dresses of fewer chains
        r2, s2, d2 = random_case(seed, 12, 40)
        check(eng, d2, CHAIN_OK)


def check_abi_wide_lines_op_count(eng):
    """a taken file may hold 2^64 - 1 in a data line: the count call of wga_chain_lines_ops says how many ops its fill call would
    write (pieces of at most 2^28 - 1 each), so that the caller's allocation fails instead of the fill running past a buffer"""
    from wgatools_amd.engine import OP_MAX_LEN
    st, bad, heads, lines, off, d_lines, d_off = check(eng, head_line(0) + b"%d %d %d\n7 0 %d\n1\n" % (U64, U64, U64, OP_MAX_LEN + 1), CHAIN_OK)
    cnt = eng.chain_lines_ops(1, 3, d_lines, d_off).numpy()
    assert int(cnt[0]) == 3 * -(-U64 // OP_MAX_LEN) + (1 + 2) + 1


# ---- command level ---------------------------------------------------------------------------------------------------------
def run(cli, *args, env=None, stdin=None):
    r = subprocess.run([cli] + list(args), input=stdin, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       env=dict(os.environ, **env) if env else None)
    err = r.stderr.decode(errors="replace").strip()
    return r.returncode, r.stdout, re.split(r" (?:ERROR|WARN) ", err, 1)[-1]       # the text after the log line's level


HOST = {"WGA_CHAIN_READER": "host"}


def both_readers(cli, *args):
    """the command under the default reader and under the host reader: the same stdout bytes, exit code and message"""
    got, host = run(cli, *args), run(cli, *args, env=HOST)
    assert got[0] in (0, 1) and host[0] in (0, 1), (args, got[0], host[0])      # finished or failed with a message: never a signal
    assert got == host, (args, got[0], host[0], got[2], host[2])
    return got


def reader_of(cli, path, env=None):
    rc, out, err = run(cli, "__chain_reader", path, env=env)
    lines = out.decode(errors="replace").split("\n")
    return lines[0], lines[1:], rc, err


def write(tmp_path, name, data):
    path = str(tmp_path / name)
    with open(path, "wb") as f:
        f.write(data)
    return path


def expected_chain2paf(recs, t_name, t_size, q_name, q_size, starts):
    out = []
    for r, (ts, qs) in zip(recs, starts):
        counts, cg = orc.parse_chain_to_cigar(r["lines"], r["neg"])
        match, mism, del_bp, inv_del_bp = counts[0], counts[1], counts[5], counts[9]
        out.append("%s\t%d\t%d\t%d\t%s\t%s\t%d\t%d\t%d\t%d\t%d\t255\tcg:Z:%s\n" % (
            q_name, q_size, qs, qs + r["q_ali"], "-" if r["neg"] else "+", t_name, t_size, ts, ts + r["t_ali"], match,
            match + mism + del_bp + inv_del_bp, cg))
    return "".join(out).encode()


def expected_filter(recs, t_name, t_size, q_name, q_size, starts, min_block, min_query):
    out = []
    for r, (ts, qs) in zip(recs, starts):
        if r["t_ali"] < min_block or q_size < min_query:
            continue
        out.append("chain\t%d\t%s\t%d\t+\t%d\t%d\t%s\t%d\t%s\t%d\t%d\t%d\n" % (
            1000 + r["id"], t_name, t_size, ts, ts + r["t_ali"], q_name, q_size, "-" if r["neg"] else "+", qs, qs + r["q_ali"], r["id"]))
        out.append("".join("%d\t%d\t%d\n" % ln for ln in r["lines"]) + "\n")
    return "".join(out).encode()


def check_reader_selection(cli, tmp_path):
    """__chain_reader: `device` for the random well-formed files, `host` under WGA_CHAIN_READER=host, the same record lines"""
    for k, (seed, n, ml) in enumerate(((11, 200, 120), (20, 12, 40), (21, 12, 40))):
        recs, starts, data = random_case(seed, n, ml)
        path = write(tmp_path, "r%d.chain" % k, data)
        dev, host = reader_of(cli, path), reader_of(cli, path, env=HOST)
        assert (dev[0], host[0]) == ("device", "host") and dev[2] == host[2] == 0
        assert dev[1] == host[1] and len(dev[1]) == n + 1
        r, (ts, qs) = recs[0], starts[0]
        assert dev[1][0] == "%d|tchr|%d|+|%d|%d|qchr|%d|%s|%d|%d|%d|%d|%d" % (
            1000 + r["id"], 10 ** 8, ts, ts + r["t_ali"], 10 ** 8, "-" if r["neg"] else "+", qs, qs + r["q_ali"], r["id"],
            len(r["lines"]), sum(sum(ln) for ln in r["lines"]))
    for name, data, bad in FALLBACKS:
        assert reader_of(cli, write(tmp_path, name + ".chain", data))[0] == "host", name
    for name, data in ACCEPTED:
        assert reader_of(cli, write(tmp_path, name + ".chain", data))[0] == ("device" if data else "host"), name


def fasta_pair(tmp_path, T=400000, Q=380000, seed=8):
    """the small FASTA pair of cli_cases.test_chain2maf_end_to_end"""
    rng = np.random.default_rng(seed)
    pools = []
    for name, n in ((b"tchr", T), (b"qchr", Q)):
        seq = np.frombuffer(b"ACGTacgtN", dtype=np.uint8)[rng.integers(0, 9, n)].tobytes()
        with open(str(tmp_path / (name.decode() + ".fa")), "wb") as f:
            f.write(b">" + name + b"\n")
            for i in range(0, n, 60):
                f.write(seq[i:i + 60] + b"\n")
        pools.append(seq)
    return str(tmp_path / "tchr.fa"), str(tmp_path / "qchr.fa"), pools[0], pools[1]


def expected_chain2maf(recs, starts, t_fa, q_fa, t_pool, q_pool, T, Q):
    out = ["#maf version=1.6 convert_from=chain t_seq_path=%s q_seq_path=%s\n" % (t_fa, q_fa)]
    for r, (ts, qs) in zip(recs, starts):
        t, q = t_pool[ts:ts + r["t_ali"]], q_pool[qs:qs + r["q_ali"]]
        if r["neg"]:
            q = orc.reverse_complement(q)
        et, eq = orc.parse_chain_to_insert(r["lines"], t, q)
        out.append("a score=255\ns\ttchr\t%d\t%d\t+\t%d\t%s\ns\tqchr\t%d\t%d\t%s\t%d\t%s\n\n" % (
            ts, r["t_ali"], T, et.decode(), Q - (qs + r["q_ali"]) if r["neg"] else qs, r["q_ali"], "-" if r["neg"] else "+", Q,
            eq.decode()))
    return "".join(out).encode()


def small_files():
    return [(n, d) for n, d, _ in FALLBACKS] + ACCEPTED + [("tok%d" % k, d) for k, d in enumerate(TOKEN_FILES)]


def check_chain2paf(cli, tmp_path):
    for k, (seed, n, ml) in enumerate(((11, 200, 120), (22, 12, 40))):
        recs, starts, data = random_case(seed, n, ml)
        path = write(tmp_path, "r%d.chain" % k, data)
        rc, out, err = both_readers(cli, "chain2paf", path)
        assert rc == 0 and out == expected_chain2paf(recs, "tchr", 10 ** 8, "qchr", 10 ** 8, starts), err
        # batches that do not start at the first chain: their offsets are rebased on the device
        assert run(cli, "chain2paf", path, env={"WGA_CHAIN_BATCH_LINES": "500"}) == (rc, out, err)
    for name, data in small_files():
        both_readers(cli, "chain2paf", write(tmp_path, name + ".chain", data))


def check_filter(cli, tmp_path):
    recs, starts, data = random_case()
    path = write(tmp_path, "r.chain", data)
    for b, q in ((0, 0), (2000, 0), (0, 10 ** 8 + 1)):
        rc, out, err = both_readers(cli, "filter", "-f", "chain", path, "-b", str(b), "-q", str(q))
        assert rc == 0 and out == expected_filter(recs, "tchr", 10 ** 8, "qchr", 10 ** 8, starts, b, q), err
    for name, data in small_files():
        both_readers(cli, "filter", "-f", "chain", write(tmp_path, name + ".chain", data), "-b", "20", "-q", "5")


def check_chain2maf(cli, tmp_path):
    T, Q = 400000, 380000
    t_fa, q_fa, t_pool, q_pool = fasta_pair(tmp_path, T, Q)
    recs, starts, data = random_case(23, 30, 120, T, Q)
    path = write(tmp_path, "r.chain", data)
    rc, out, err = both_readers(cli, "chain2maf", path, "--target", t_fa, "--query", q_fa)
    assert rc == 0 and out == expected_chain2maf(recs, starts, t_fa, q_fa, t_pool, q_pool, T, Q), err
    for name, data in small_files():
        both_readers(cli, "chain2maf", write(tmp_path, name + ".chain", data), "-g", t_fa, "-q", q_fa)


ATOMS = [b"\r", b"\t", b" ", b"\n", b"x", b"c", b"chain", b"-1", b"1e3", b"#", "\u00e9".encode(), None]      # None: a newline deleted
N_DIFF = 300


def diff_file(i):
    """file i of the differential run: (text, well-formed); even i well-formed, odd i with one atom put in at a random place"""
    recs, starts, data = random_case(1000 + i, 3, 6)
    if i % 2 == 0:
        return data, True
    rng = random.Random(5000 + i)
    atom = ATOMS[rng.randrange(len(ATOMS))]
    if atom is None:
        at = rng.choice([k for k, c in enumerate(data) if c == 0x0A])
        return data[:at] + data[at + 1:], False
    at = rng.randrange(len(data) + 1)
    return data[:at] + atom + data[at:], False


def check_differential(cli, tmp_path, lo, hi):
    """files [lo, hi) of the 300: the well-formed half reports `device`; chain2paf is the same under both readers for all"""
    for i in range(lo, hi):
        data, good = diff_file(i)
        path = write(tmp_path, "d%d.chain" % i, data)
        if good:
            assert reader_of(cli, path)[0] == "device", i
        rc, out, err = both_readers(cli, "chain2paf", path)
        assert not good or (rc == 0 and out.count(b"\n") == 3), (i, err)


def check_gpus(cli, tmp_path, gpus=2):
    """--gpus N to a plain file: the bytes of one device, for a good file and one whose 7th chain fails in the walk"""
    T, Q = 400000, 380000
    t_fa, q_fa, t_pool, q_pool = fasta_pair(tmp_path, T, Q)
    recs, starts, data = random_case(24, 25, 60, T, Q)
    broken = [dict(r) for r in recs]
    broken[6]["t_ali"] -= 40
    broken[6]["q_ali"] -= 40
    broken[6]["lines"] = broken[6]["lines"][:-1] + [(broken[6]["lines"][-1][0], 3, 0), (1, 0, 0)]
    bad = random_text(broken, b"tchr", T, b"qchr", Q, starts, 26)
    for name, text, rc_want in (("good", data, 0), ("bad", bad, 1)):
        path = write(tmp_path, name + ".chain", text)
        assert reader_of(cli, path)[0] == "device"
        for args in (("chain2paf", path), ("chain2maf", path, "-g", t_fa, "-q", q_fa)):
            res = []
            for g in (1, gpus):
                outp = str(tmp_path / ("out%d" % g))
                rc, _, err = run(cli, "--gpus", str(g), *args, "-o", outp, "-r")
                res.append((rc, open(outp, "rb").read(), err))
                hrc, _, herr = run(cli, "--gpus", str(g), *args, "-o", outp, "-r", env=HOST)
                assert (hrc, open(outp, "rb").read(), herr) == res[-1], (name, args[0], g)
            assert res[0] == res[1], (name, args[0])
            assert res[0][0] == (rc_want if args[0] == "chain2maf" else 0), res[0][2]
            if args[0] == "chain2maf":
                n_ok = len(recs) if name == "good" else 6
                assert res[0][1] == expected_chain2maf(recs[:n_ok], starts[:n_ok], t_fa, q_fa, t_pool, q_pool, T, Q)
