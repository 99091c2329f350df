"""`filter -f paf` on the device (K24): the C-ABI entries (Engine.paf_split -> Engine.paf_filter / Engine.paf_pairs) and the
`wgatools filter -f paf` command with its device path against its host path.  The expectation is maf_rewrite_ref.filter_paf /
filter_paf_pairs, the restatement of the reference with full csv semantics.  Imported by test_emu_paf_filter.py (emulator
build, CPU) and test_gpu_paf_filter.py (the product on a GPU); each provides the `cli` and `eng` fixtures."""
import gzip
import os
import random
import re
import subprocess

import numpy as np

import maf_rewrite_ref as ref
from wgatools_amd.engine import PAF_FILTER_TILE, PAF_LINE_DTYPE, PAF_OK, PAF_SKIP

U64 = (1 << 64) - 1
T = PAF_FILTER_TILE
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "testdotplot.paf")


# ---- texts ---------------------------------------------------------------------------------------------------------------------
def paf_line(q=b"q1", ql=1000, qs=0, qe=100, strand=b"+", t=b"t1", tl=2000, ts=10, te=110, m=90, bl=100, mq=60, tags=(b"tp:A:P",),
             end=b"\n"):
    """one PAF line; the numbers may be given as bytes (`+5`, `007`)"""
    f = [q, ql, qs, qe, strand, t, tl, ts, te, m, bl, mq] + list(tags)
    return b"\t".join(x if isinstance(x, bytes) else b"%d" % x for x in f) + end


def line_of_len(n, **kw):
    """a line of exactly n bytes, its newline included: a cg:Z: tag of `=` ops takes up the slack"""
    base = paf_line(tags=(b"cg:Z:",), **kw)
    pad = n - len(base)
    assert pad >= 2, (n, len(base))
    return paf_line(tags=(b"cg:Z:" + b"9" * (pad - 1) + b"=",), **kw)


def cigar(rng, n_ops):
    return b"".join(b"%d%s" % (rng.randrange(1, 2000), rng.choice([b"=", b"X", b"I", b"D", b"M"])) for _ in range(n_ops))


def random_file(seed, n_lines=300, names=4, cg_bytes=(None, 5, 100, 9000, 40000), skip=0.05, end=True):
    """canonical lines: names from a small alphabet, cg:Z: tags of very different lengths, some comment and blank lines"""
    rng = random.Random(seed)
    out = []
    for k in range(n_lines):
        if rng.random() < skip:
            out.append(rng.choice([b"\n", b"#comment %d\n" % k, b"#\n"]))
            continue
        want = rng.choice(cg_bytes)
        tags = [b"tp:A:P", b"NM:i:%d" % rng.randrange(50)]
        if want is not None:
            cg = cigar(rng, max(1, want // 4))[:want]
            tags.insert(rng.randrange(3), b"cg:Z:" + cg.rstrip(b"0123456789") + (b"" if cg[-1:] in b"=XIDM" else b"="))
        ts = rng.randrange(0, 10 ** 6)
        out.append(paf_line(q=b"q" + rng.choice(b"abcd"[:names].decode()).encode() * rng.randrange(1, 4), ql=rng.randrange(0, 5000),
                            qs=rng.randrange(100), qe=rng.randrange(100, 200), strand=rng.choice([b"+", b"-"]),
                            t=b"chr" + rng.choice(b"1234"[:names].decode()).encode(), tl=10 ** 7, ts=ts, te=ts + rng.randrange(0, 3000),
                            m=rng.randrange(100), bl=rng.randrange(100, 200), mq=rng.randrange(61), tags=tags))
    data = b"".join(out)
    return data if end else data.rstrip(b"\n") + b"\tzz:Z:last"


# ---- ABI level -----------------------------------------------------------------------------------------------------------------
def split(eng, data):
    """(d_text, n_lines, d_lines) of Engine.paf_split"""
    d_text = eng.upload(np.frombuffer(data + b"\0" * 16, dtype=np.uint8))
    n = eng.paf_split(d_text, len(data))
    d_lines = eng.empty(n + 1, PAF_LINE_DTYPE)
    assert eng.paf_split(d_text, len(data), d_lines) == n
    return d_text, n, d_lines


def filt(eng, data, b=0, q=0, sp=None):
    d_text, n, d_lines = sp or split(eng, data)
    return eng.paf_filter(d_text, len(data), d_lines, n, b, q)          # the guards around d_out are checked in there


def check(eng, data, b=0, q=0, sp=None):
    """an exact text: the device's bytes are the restatement's"""
    text, kept, bad = filt(eng, data, b, q, sp)
    exp = ref.filter_paf(data, b, q)
    assert bad is None, (bad, data[:200])
    assert kept == exp.count(b"\n") and text == exp, (b, q, kept, len(text), len(exp), data[:200])
    return text


def check_inexact(eng, data, line, b=0, q=0):
    text, kept, bad = filt(eng, data, b, q)
    assert (text, bad) == (b"", line), (bad, line, data[:200])


def check_abi_tile_and_group_edges(eng):
    short = [paf_line(q=b"s%d" % k, ts=k, te=k + 50) for k in range(8)]
    for d1 in (-1, 0, 1):                     # the first kept line ends at T - 1, T, T + 1: the second one starts there
        for d2 in (-1, 0, 1):                 # ... and ends at 15 / 16 / 17 within a 16-byte group
            data = line_of_len(T + d1) + line_of_len(80 - (T + d1) % 16 + d2, q=b"x") + b"".join(short) + \
                line_of_len(2 * T - 7 + d2, q=b"y") + short[0]
            assert check(eng, data) == data
            # the same places with dropped lines between the kept ones
            drop = paf_line(q=b"gone", ts=5, te=6)
            mixed = drop + line_of_len(T + d1) + drop * 3 + line_of_len(80 - (T + d1) % 16 + d2, q=b"x") + drop + short[1] + drop
            check(eng, mixed, b=20)
    for lead in range(0, 48, 5):              # a short line straddles the tile's edge byte by byte
        data = line_of_len(T - 30 - lead) + b"".join(short)
        assert check(eng, data) == data
    long_line = line_of_len(5 * T // 2 + 3, q=b"long", ts=0, te=10 ** 6)       # 2.5 tiles between 60-byte lines
    data = b"".join(short[:4]) + long_line + b"".join(short[4:])
    assert check(eng, data) == data
    assert check(eng, data, b=1000) == long_line
    assert check(eng, data, b=51) == long_line
    alt = b"".join(paf_line(q=b"a%d" % k, ts=0, te=(100 if k % 2 else 10), tags=(b"cg:Z:" + b"7=" * (k % 37),)) for k in range(700))
    assert len(alt) > 40000
    text = check(eng, alt, b=50)                                               # kept / dropped alternating
    assert text.count(b"\n") == 350
    assert filt(eng, alt, b=101) == (b"", 0, None)                             # nothing kept
    assert check(eng, alt) == alt                                              # everything kept: the input's bytes
    assert check(eng, alt[:-1]) == alt                                         # an unterminated last line gains its newline
    assert check(eng, alt[:-1], b=50).count(b"\n") == 350
    assert check(eng, alt + paf_line(ts=0, te=1, end=b""), b=50).count(b"\n") == 350      # ... and a dropped one leaves nothing
    inter = b"#head\n\n" + b"".join(ln + (b"\n" if k % 3 == 0 else b"#c%d\n" % k if k % 3 == 1 else b"") for k, ln in enumerate(short * 40))
    assert check(eng, inter) == b"".join(short * 40)                           # `#` and blank lines interleaved
    check(eng, inter + b"#no newline at the end")
    assert filt(eng, b"") == (b"", 0, None)                                    # n_lines == 0
    assert filt(eng, b"\n\n#x\n") == (b"", 0, None)
    for n in (255, 256, 257, 1024, 1025):                                      # the line passes' and the scan's blocks
        data = b"".join(paf_line(q=b"n%d" % k, ts=0, te=k % 7) for k in range(n))
        assert check(eng, data) == data
        check(eng, data, b=3)


def check_abi_thresholds(eng):
    ln = paf_line(ql=777, ts=100, te=350)
    assert check(eng, ln, b=250, q=777) == ln
    assert check(eng, ln, b=251, q=777) == b""
    assert check(eng, ln, b=250, q=778) == b""
    assert check(eng, ln, b=251, q=778) == b""
    wrap = paf_line(ts=100, te=0)                                              # target_end < target_start: the span wraps
    assert check(eng, wrap, b=(1 << 64) - 100) == wrap
    assert check(eng, wrap, b=(1 << 64) - 99) == b""
    big = paf_line(ql=U64, ts=0, te=U64)
    assert check(eng, big, b=U64, q=U64) == big


NUM_COLS = (1, 2, 3, 6, 7, 8, 9, 10, 11)


def with_field(col, value):
    f = paf_line().rstrip(b"\n").split(b"\t")
    f[col] = value
    return b"\t".join(f) + b"\n"


def check_abi_exactness(eng):
    good = paf_line(q=b"g")
    for col in NUM_COLS:
        for v in (b"+5", b"007", b"00"):
            data = good * 3 + with_field(col, v) + good
            assert ref.filter_paf(data, 0, 0) != data                          # the reference would write other bytes
            check_inexact(eng, data, 3)
        for v in (b"0", b"10"):
            data = good * 3 + with_field(col, v) + good
            assert check(eng, data) == data
    check(eng, good + with_field(0, b"007") + with_field(5, b"+5") + with_field(12, b"007") + with_field(4, b"-"))       # names, tags
    hi = b"\xc3\xa9"
    check_inexact(eng, good * 2 + paf_line(q=b"caf" + hi) + good, 2)
    check_inexact(eng, good * 2 + paf_line(tags=(b"tp:A:P", b"zz:Z:" + hi)) + good, 2)
    check_inexact(eng, good + b"#comm" + hi + b"ent\n" + good, 1)
    check_inexact(eng, good * 5 + paf_line(q=b"x" + hi, end=b""), 5)         # in an unterminated last line
    check_inexact(eng, good * 2 + with_field(7, b"007") + good * 300 + with_field(2, b"+1"), 2)      # the lower index, across blocks
    check_inexact(eng, good * 2 + paf_line(q=b"h" + hi) + good * 300 + with_field(2, b"+1"), 2)
    check_inexact(eng, good * 300 + with_field(2, b"+1") + paf_line(q=b"h" + hi), 300)
    check_inexact(eng, good + b"a\tb\tc\n" + good, 1)                        # a fallback line of the splitter: short
    check_inexact(eng, good + paf_line(q=b'"quoted"') + good, 1)
    check_inexact(eng, good + paf_line(end=b"\r\n") + good, 1)
    check_inexact(eng, good * 2 + with_field(7, b"007"), 2, b=10 ** 6)       # inexact lines count, kept or not
    big = good * 3 + with_field(1, b"00") + line_of_len(3 * T)
    check_inexact(eng, big, 3)


def check_abi_random_files(eng, seeds=range(12)):
    for seed in seeds:
        data = random_file(seed, end=seed % 3 != 0)
        assert 10000 < len(data) < (1 << 22)
        sp = split(eng, data)
        for b, q in ((0, 0), (1500, 0), (700, 2500)):
            check(eng, data, b, q, sp)


def py_pairs(data):
    """(pairs in first-appearance order as [first_line, sum, qname, tname], pair_of_line) from a dict"""
    lines = data.split(b"\n")
    if lines[-1] == b"":
        lines.pop()
    idx, pairs, pol = {}, [], []
    for i, ln in enumerate(lines):
        if not ln or ln.startswith(b"#"):
            pol.append(0xFFFFFFFF)
            continue
        f = ln.split(b"\t")
        key = (f[0], f[5])
        if key not in idx:
            idx[key] = len(pairs)
            pairs.append([i, 0, f[0], f[5]])
        p = pairs[idx[key]]
        p[1] = (p[1] + ((int(f[8]) - int(f[7])) & U64)) & U64
        pol.append(idx[key])
    return pairs, pol


def check_pairs(eng, data, n_pairs=None):
    d_text, n, d_lines = split(eng, data)
    st = d_lines.numpy()[:n]["status"]
    assert set(st.tolist()) <= {PAF_OK, PAF_SKIP}
    pairs, d_pol = eng.paf_pairs(d_text, len(data), d_lines, n)
    exp, exp_pol = py_pairs(data)
    assert n_pairs is None or len(exp) == n_pairs
    assert len(pairs) == len(exp)
    assert d_pol.numpy().tolist() == exp_pol
    assert pairs["first_line"].tolist() == [e[0] for e in exp]
    assert pairs["sum"].tolist() == [e[1] for e in exp]
    for p, e in zip(pairs, exp):
        assert data[int(p["qname_off"]):int(p["qname_off"]) + int(p["qname_len"])] == e[2]
        assert data[int(p["tname_off"]):int(p["tname_off"]) + int(p["tname_len"])] == e[3]
    # pair mode of the filter with a keep mask made from those sums
    sums = sorted(set(int(s) for s in pairs["sum"]))
    for a in sorted({0, sums[len(sums) // 2] if sums else 0, (sums[-1] + 1) & U64 if sums else 1}):
        keep = (pairs["sum"] >= np.uint64(a)).astype(np.uint8)
        d_keep = eng.upload(np.concatenate([keep, np.zeros(16, dtype=np.uint8)]))
        text, kept, bad = eng.paf_filter(d_text, len(data), d_lines, n, pair_of_line=d_pol, pair_keep=d_keep)
        want = ref.filter_paf_pairs(data, a)
        assert bad is None and text == want and kept == want.count(b"\n"), (a, kept, len(text), len(want))
    return pairs


def pair_files():
    def L(q, t, span, k=0):
        return paf_line(q=q, t=t, ts=k, te=k + span)
    files = []
    files.append((b"".join([L(b"chrom", b"target", 5), L(b"chrom1", b"target", 7), L(b"chro", b"target", 11), L(b"chrom", b"targes", 13),
                            L(b"chrom", b"target", 17), L(b"chrom", b"targeT", 19), L(b"chroM", b"target", 23), L(b"chrom1", b"target", 29)]), 6))
    files.append((b"".join(L(b"q", b"t%d" % (k % 5), k + 1) for k in range(40)), 5))            # one query, several targets
    files.append((L(b"ab", b"c", 1) + L(b"a", b"bc", 2) + L(b"ab", b"c", 4) + L(b"a", b"bc", 8) + L(b"abc", b"", 16) + L(b"", b"abc", 32), 4))
    files.append((L(b"", b"", 1) + L(b"", b"t", 2) + L(b"q", b"", 4) + b"#c\n\n" + L(b"", b"", 8) + L(b"q", b"", 16), 3))      # empty names
    return files


def check_abi_pairs(eng):
    for data, n in pair_files():
        check_pairs(eng, data, n)
    check_pairs(eng, b"#only\n\n", 0)
    d_text, n, d_lines = split(eng, b"")
    pairs, pol = eng.paf_pairs(d_text, 0, d_lines, 0)
    assert len(pairs) == 0
    for seed in (1, 2):
        check_pairs(eng, random_file(seed, cg_bytes=(None, 5, 100)))


def one_pair_file(span=1 << 63):
    return b"".join(paf_line(q=b"only", t=b"pair", ts=0, te=span, m=k) for k in range(2000))


def many_pairs_file():
    return b"".join(paf_line(q=b"q%d" % (k % 5000 // 70), t=b"t%d" % (k % 5000 % 70), ts=k, te=2 * k + 1) for k in range(6000))


def check_abi_pairs_large(eng, hash_bits=64):
    """one pair on 2 000 lines whose sum wraps; 5 000 pairs in 6 000 lines.  hash_bits = 2: every pair starts at one of four slots"""
    eng.set_param("paf_pair_hash_bits", hash_bits)
    try:
        assert eng.get_param("paf_pair_hash_bits") == hash_bits
        pairs = check_pairs(eng, one_pair_file(), 1)
        assert int(pairs["sum"][0]) == 0                                        # 2000 * 2^63 mod 2^64
        pairs = check_pairs(eng, one_pair_file((1 << 63) + 3), 1)
        assert int(pairs["sum"][0]) == 6000
        check_pairs(eng, many_pairs_file(), 5000)
    finally:
        eng.set_param("paf_pair_hash_bits", 64)


# ---- the restatement itself (CPU) --------------------------------------------------------------------------------------------------
def check_reference_properties():
    gold = open(GOLDEN, "rb").read()
    assert ref.filter_paf(gold, 0, 0) == gold
    odd = paf_line(q=b"", t=b"", tags=(b"tp:A:P", b""))                        # empty names, an empty trailing tag
    assert ref.filter_paf(odd, 0, 0) == odd
    assert ref.filter_paf(odd[:-1], 0, 0) == odd                               # an unterminated last line gains its newline
    for col in NUM_COLS:
        for v in (b"+5", b"007", b"00"):
            assert ref.filter_paf(with_field(col, v), 0, 0) != with_field(col, v)
        for v in (b"0", b"10"):
            assert ref.filter_paf(with_field(col, v), 0, 0) == with_field(col, v)
    two = paf_line(q=b"ab", t=b"c", ts=0, te=5) + paf_line(q=b"a", t=b"bc", ts=0, te=7)
    assert ref.filter_paf_pairs(two, 6) == paf_line(q=b"a", t=b"bc", ts=0, te=7)
    assert ref.filter_paf_pairs(two, 5) == two


# ---- command level -----------------------------------------------------------------------------------------------------------------
HOST = {"WGA_PAF_READER": "host"}


def run(cli, *args, env=None, stdin=None):
    r = subprocess.run([cli] + list(args), input=stdin, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       env=dict(os.environ, **env) if env else None)
    err = r.stderr.decode(errors="replace").strip()
    return r.returncode, r.stdout, [re.split(r" (?:ERROR|WARN) ", ln, 1)[-1] for ln in err.split("\n") if ln]


def write(tmp_path, name, data):
    path = str(tmp_path / name)
    with open(path, "wb") as f:
        f.write(data)
    return path


def paths_of(cli, path, env=None):
    rc, out, err = run(cli, "__paf_filter_path", path, env=env)
    assert rc == 0, err
    return out.decode().split()


def four_piece_file(bad=None):
    """four pieces under WGA_CHUNK_BYTES=4000 (a piece ends behind the first line end at or after 4000 bytes); `bad` goes into
    the third"""
    piece = [b"".join(paf_line(q=b"p%dq%d" % (p, k % 3), t=b"t%d" % (k % 2), ts=k, te=3 * k + p) for k in range(70)) for p in range(4)]
    for p in piece:
        assert 3000 < len(p) < 4000
    rows = [p + line_of_len(1200, q=b"fill") for p in piece]
    if bad is not None:
        rows[2] = piece[2][:1500].rsplit(b"\n", 1)[0] + b"\n" + bad + piece[2][1500:].split(b"\n", 1)[1] + line_of_len(1200, q=b"fill")
    return b"".join(rows)


def cli_random_file(seed, end=True):
    """a random canonical file for the command-level cases: fewer lines than the ABI cases', still from 60 bytes to 9 KB"""
    return random_file(seed, n_lines=60, cg_bytes=(None, 5, 100, 9000), end=end)


def check_path_selection(cli, tmp_path):
    for seed in (0, 1):
        path = write(tmp_path, "r%d.paf" % seed, cli_random_file(seed))
        assert paths_of(cli, path) == ["device"]
        assert paths_of(cli, path, env=HOST) == ["host"]
        many = paths_of(cli, path, env={"WGA_CHUNK_BYTES": "4000"})
        assert len(many) > 5 and set(many) == {"device"}
    assert paths_of(cli, write(tmp_path, "quote.paf", paf_line() * 3 + paf_line(q=b'"q"') + paf_line())) == ["host"]
    assert paths_of(cli, write(tmp_path, "007.paf", paf_line() * 3 + with_field(7, b"007") + paf_line())) == ["host"]
    chunk = CHUNK
    assert paths_of(cli, write(tmp_path, "four.paf", four_piece_file()), env=chunk) == ["device"] * 4
    assert paths_of(cli, write(tmp_path, "four7.paf", four_piece_file(with_field(7, b"007"))), env=chunk) == ["device", "device", "host", "device"]
    assert paths_of(cli, write(tmp_path, "four7.paf", four_piece_file(with_field(7, b"007"))), env=dict(chunk, **HOST)) == ["host"] * 4
    assert paths_of(cli, write(tmp_path, "empty.paf", b"")) == []


def byte_files():
    """name -> (text, the text is small: it also runs in pieces of one line)"""
    return {"r0": (cli_random_file(0), False), "r1": (cli_random_file(1, end=False), False),
            "gold": (open(GOLDEN, "rb").read(), True), "small": (random_file(5, n_lines=40, cg_bytes=(None, 5, 100)), True),
            "four": (four_piece_file(), False), "four7": (four_piece_file(with_field(7, b"007")), False),
            "quote": (paf_line(ts=0, te=20) + paf_line(q=b"q2", ts=0, te=30) + paf_line() + paf_line(q=b'"q"', tags=(b'zz:Z:"a""b"',)) +
                      paf_line(ts=0, te=5000), True)}


BYTE_FILES = ("r0", "r1", "gold", "small", "four", "four7", "quote")
CHUNK = {"WGA_CHUNK_BYTES": "4000"}


def check_bytes(cli, tmp_path, name):
    """device run == host run == the restatement: from a path and from stdin, in pieces, into a `.gz` file"""
    data, small = byte_files()[name]
    path = write(tmp_path, name + ".paf", data)
    spans = sorted((int(f[8]) - int(f[7])) & U64 for f in ref.csv_records(data))
    b, q = spans[len(spans) // 2], 0
    want = ref.filter_paf(data, b, q)
    assert want and want != ref.filter_paf(data, 0, 0)
    args = ("filter", "-f", "paf", "-b", str(b), "-q", str(q))
    for chunk in ("64", "4000", None) if small else ("4000", None):
        env = {"WGA_CHUNK_BYTES": chunk} if chunk else {}
        assert run(cli, *args, path, env=env) == (0, want, []), (name, chunk)
        assert run(cli, *args, path, env=dict(env, **HOST)) == (0, want, []), (name, chunk)
    assert run(cli, *args, stdin=data, env=CHUNK) == (0, want, []), name
    assert run(cli, "filter", "-f", "paf", path) == (0, ref.filter_paf(data, 0, 0), []), name            # thresholds 0: one count call
    assert run(cli, "filter", "-f", "paf", "-q", "2500", path, env=CHUNK) == (0, ref.filter_paf(data, 0, 2500), []), name
    gz = str(tmp_path / (name + ".out.paf.gz"))
    assert run(cli, *args, path, "-o", gz, "-r", env=CHUNK)[0] == 0
    assert gzip.open(gz, "rb").read() == want, name


def check_min_align(cli, tmp_path, name):
    data, small = byte_files()[name]
    path = write(tmp_path, name + ".paf", data)
    total = {}
    for f in ref.csv_records(data):
        total[(f[0], f[5])] = (total.get((f[0], f[5]), 0) + ((int(f[8]) - int(f[7])) & U64)) & U64
    sums = sorted(total.values())
    mid = sums[len(sums) // 2]
    want = ref.filter_paf_pairs(data, mid)
    assert want
    args = ("filter", "-f", "paf", "-b", "99999999", "-a")
    for chunk in ("64", "4000", None) if small else ("4000", None):             # one resident piece, or many of either path
        env = {"WGA_CHUNK_BYTES": chunk} if chunk else {}
        for e in (env, dict(env, **HOST)):
            assert run(cli, *args, str(mid), path, env=e) == (0, want, [ref.PAF_ALIGN_WARNING]), (name, chunk, e)
    assert run(cli, *args, str(mid), stdin=data, env=CHUNK) == (0, want, [ref.PAF_ALIGN_WARNING]), name
    assert ref.filter_paf_pairs(data, 0) == ref.filter_paf(data, 0, 0)
    assert run(cli, *args, "0", path) == (0, ref.filter_paf(data, 0, 0), [ref.PAF_ALIGN_WARNING]), name      # `-a 0` keeps every record
    assert run(cli, *args, str(sums[-1] + 1), path, env=CHUNK) == (0, b"", [ref.PAF_ALIGN_WARNING]), name


def check_min_align_wraps(cli, tmp_path):
    """one pair on 2 000 lines whose sum wraps to 6 000, next to a pair of 5 999"""
    wrap = write(tmp_path, "wrap.paf", one_pair_file((1 << 63) + 3) + paf_line(q=b"other", ts=0, te=5999))
    for a, n in ((6000, 2000), (6001, 0), (5999, 2001)):
        rc, out, err = run(cli, "filter", "-f", "paf", "-a", str(a), wrap)
        assert rc == 0 and out.count(b"\n") == n and out == ref.filter_paf_pairs(open(wrap, "rb").read(), a)


def check_error_order(cli, tmp_path):
    """an 11-field line in the third piece: the records in front of that piece are written, then the host reader's message"""
    short = b"\t".join(paf_line().split(b"\t")[:11]) + b"\n"
    data = four_piece_file(short)
    path = write(tmp_path, "short.paf", data)
    chunk = {"WGA_CHUNK_BYTES": "4000"}
    assert paths_of(cli, path, env=chunk)[:2] == ["device", "device"]
    fill = line_of_len(1200, q=b"fill")
    front = data[:data.index(fill, data.index(fill) + 1) + len(fill)]            # the first two pieces
    n_before = data[:data.index(short)].count(b"\n")                           # the records in front of the short line
    for b in (0, 100):
        got = run(cli, "filter", "-f", "paf", "-b", str(b), path, env=chunk)
        assert got == run(cli, "filter", "-f", "paf", "-b", str(b), path, env=dict(chunk, **HOST))
        assert got[0] == 1 and got[1] == ref.filter_paf(front, b, 0) and got[1]
        assert "invalid length 11" in got[2][-1] and "record %d " % n_before in got[2][-1], got[2]
    got = run(cli, "filter", "-f", "paf", "-a", "0", path, env=chunk)
    assert got == run(cli, "filter", "-f", "paf", "-a", "0", path, env=dict(chunk, **HOST))
    assert got[0] == 1 and got[1] == b"" and got[2][0] == ref.PAF_ALIGN_WARNING and "invalid length 11" in got[2][-1]


def check_gpus(cli, tmp_path, gpus=2):
    data = four_piece_file()
    path = write(tmp_path, "g.paf", data)
    for args in (("-b", "100"), ("-a", "800")):
        one = run(cli, "filter", "-f", "paf", *args, path)
        assert one[0] == 0 and one[1]
        assert run(cli, "--gpus", str(gpus), "filter", "-f", "paf", *args, path) == one
        assert run(cli, "--gpus", str(gpus), "filter", "-f", "paf", *args, path, env={"WGA_CHUNK_BYTES": "4000"}) == one
