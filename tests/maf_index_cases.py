"""`maf-index` on the device (K35): the C-ABI entry (Engine.maf_index over wga_maf_split's table) against maf_index_ref group by
group, and the command with its device writer against WGA_MAF_INDEX_WRITER=host and the restatement, byte for byte.
Imported by test_emu_maf_index.py (emulator build, CPU) and test_gpu_maf_index.py (the product on a GPU); each provides the `cli`
and `eng` fixtures."""
import ctypes as C
import os
import random
import shutil

import numpy as np

import maf2paf_cases as m2p
import maf_ext_cases as mext
import maf_ext_ref as mref
import maf_index_ref as ref
from helpers import GOLDEN
from maf_chunk_cases import maf_text, random_blocks, run
from wgatools_amd.engine import MAF_LINE_DTYPE, E_FALLBACK

U64 = (1 << 64) - 1
E_INVALID_ARG = -1
SLINE_COUNTS = (0, 1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 1030)     # the wave, block and scan-partial borders
HOST_WRITER = {"WGA_MAF_INDEX_WRITER": "host"}
DEVICE_PHASE, HOST_PHASE = "maf-index entries (device)", "maf-index entries (host)"
HEADER = b"##maf version=1\n"


# ---- pieces ------------------------------------------------------------------------------------------------------------------------
def sline(name, start=5, asize=3, strand=b"+", size=1000, seq=b"ACG"):
    return b"s %s %d %d %s %d %s\n" % (name, start, asize, strand, size, seq)


def block(*names, start=5, between=b"\n"):
    return b"a score=1\n" + b"".join(sline(n, start + 7 * k, 2 + k, b"-" if k % 3 == 2 else b"+", 900 + len(n)) for k, n in enumerate(names)) + between


def counted_piece(n_slines, seed=0, refs=5, queries=23):
    """a piece of exactly n_slines s-lines in blocks of 1 .. 5 rows: a reference name in front, query names behind it, no name twice
    in a block, noise lines between the blocks"""
    rnd = random.Random(500 + seed)
    out, left = [HEADER], n_slines
    while left:
        rows = min(left, rnd.randint(1, 5))
        qs = rnd.sample(range(queries), rows - 1)
        out.append(block(b"ref%d" % rnd.randrange(refs), *(b"qry.%d" % q for q in qs), start=rnd.randrange(10 ** rnd.randint(1, 9)),
                         between=rnd.choice((b"\n", b"\n\n", b"# note\n\n", b"i x C 0 C 0\n\n", b"e y 1 2 + 3 I\n"))))
        left -= rows
    return b"".join(out)


class Split:
    """a piece on the device with wga_maf_split's table"""

    def __init__(self, eng, piece):
        self.piece, self.n_bytes = piece, len(piece)
        self.d_text = eng.upload(np.frombuffer(piece + b"\0" * 16, dtype=np.uint8))
        self.n_lines = eng.maf_split(self.d_text, len(piece)) if piece else 0
        self.d_lines = eng.empty(self.n_lines + 1, MAF_LINE_DTYPE)
        if piece:
            assert eng.maf_split(self.d_text, len(piece), self.d_lines) == self.n_lines

    def args(self):
        return self.d_text, self.n_bytes, self.d_lines, self.n_lines


def compare(piece, got, want):
    """Engine.maf_index's result against maf_index_ref.piece_index, group by group"""
    for k in ("n_blocks", "n_slines", "first_dup_line", "first_conflict_line", "next_offset"):
        assert got[k] == want[k], (k, got[k], want[k])
    names, text = got["names"], got["text"]
    assert got["n_names"] == len(want["groups"])
    if not want["n_slines"]:
        assert text == b"" and len(names) == 0
        return
    assert len(names) == len(want["groups"]) + 1
    at = 0
    for g, (name, size, isref, first_line, ivls) in enumerate(want["groups"]):
        e = names[g]
        assert piece[int(e["name_off"]):int(e["name_off"]) + int(e["name_len"])] == name, g
        assert (int(e["size"]), int(e["isref"]), int(e["first_line"]), int(e["n_ivls"])) == (size, int(isref), first_line, len(ivls)), (g, name)
        exp = b",".join(ivls)
        assert int(e["text_off"]) == at and text[at:at + len(exp)] == exp, (g, name, text[at:at + len(exp) + 20], exp)
        at += len(exp)
    last = names[len(want["groups"])]
    assert int(last["text_off"]) == at == len(text)
    assert all(int(last[f]) == 0 for f in ("name_off", "size", "first_line", "n_ivls", "name_len", "isref"))


def check_piece(eng, piece, skip=0, base=0, carry=0, shift=0):
    s = Split(eng, piece)
    got = eng.maf_index(*s.args(), skip=skip, base=base, carry_offset=carry, out_shift=shift)
    assert got is not None
    compare(piece, got, ref.piece_index(piece, skip, base, carry))
    return got


# ---- the C-ABI entry ---------------------------------------------------------------------------------------------------------------
def check_abi_sline_counts(eng, counts=SLINE_COUNTS):
    for n in counts:
        got = check_piece(eng, counted_piece(n, seed=n), shift=n % 16)
        assert got["n_slines"] == n and got["first_dup_line"] is None and got["first_conflict_line"] is None


def with_param(eng, name, value, default, fn):
    eng.set_param(name, value)
    try:
        assert eng.get_param(name) == value
        return fn()
    finally:
        eng.set_param(name, default)


def check_abi_hash_collisions(eng):
    """maf_index_hash_bits = 1: two start slots for all names, the bytes decide; names that differ only in their last byte or only
    in their length"""
    near = [b"a", b"ab", b"abc", b"abd", b"ab.", b"b", b"ba", b"aa", b"aaa", b"aaaa", b"chr1", b"chr10", b"chr11", b"chr2"]
    many = near + [b"n%d" % k for k in range(40)]
    rnd = random.Random(35)
    out = [HEADER]
    for _ in range(120):
        out.append(block(b"R" + rnd.choice(near), *rnd.sample(many, rnd.randint(0, 4)), start=rnd.randrange(10 ** 6)))
    piece = b"".join(out)
    plain = check_piece(eng, piece)
    cut = with_param(eng, "maf_index_hash_bits", 1, 64, lambda: check_piece(eng, piece))
    assert cut["text"] == plain["text"] and cut["names"].tobytes() == plain["names"].tobytes()
    assert plain["n_names"] > 60
    for bad in (0, 65):
        assert eng.lib.wga_ctx_set_param(eng.ctx, b"maf_index_hash_bits", bad) == E_INVALID_ARG


def interleaved_piece(n_groups, rounds=6):
    """n_groups names in blocks of three, dealt out so that every name's intervals lie far apart and between those of all others: a
    sort that is not stable, or that drops a digit, puts an interval out of file order"""
    names = [b"g%03d" % k for k in range(n_groups - 1)]                     # and the reference row `R` of every block
    out, start = [HEADER], 1
    for r in range(rounds):
        order = names[r % len(names):] + names[:r % len(names)]
        if r % 2:
            order.reverse()
        for k in range(0, len(order), 3):
            out.append(b"a\n" + sline(b"R", start + 5) + b"".join(sline(b"q" + n, start + j) for j, n in enumerate(order[k:k + 3])) + b"\n")
            start += 10
    return b"".join(out)


def check_abi_sort_passes(eng, groups=(4, 5, 16, 17, 65)):
    """maf_index_sort_bits = 2: one digit pass for 4 groups, two for 5 and 16, three for 17, four for 65; the default width"""
    for n in groups:
        piece = interleaved_piece(n)
        wide = check_piece(eng, piece)
        assert wide["n_names"] == n
        for bits in (2, 1, 3):
            narrow = with_param(eng, "maf_index_sort_bits", bits, 8, lambda: check_piece(eng, piece))
            assert narrow["text"] == wide["text"] and narrow["names"].tobytes() == wide["names"].tobytes(), (n, bits)
    if 65 in groups:                                                        # more than one block of the sort, four passes
        piece = interleaved_piece(65, rounds=26)
        wide = check_piece(eng, piece)
        assert wide["n_slines"] > 2048
        narrow = with_param(eng, "maf_index_sort_bits", 2, 8, lambda: check_piece(eng, piece))
        assert narrow["text"] == wide["text"] and narrow["names"].tobytes() == wide["names"].tobytes()
    for bad in (0, 9):
        assert eng.lib.wga_ctx_set_param(eng.ctx, b"maf_index_sort_bits", bad) == E_INVALID_ARG


def check_abi_offsets(eng):
    b1, b2, b3 = block(b"r", b"x"), block(b"r", b"y", start=50), block(b"r", b"x", b"y", start=90)
    long_note = b"# " + b"n" * 5000 + b"\n"
    cases = [
        HEADER + b1,                                                        # a block right behind the header
        HEADER + b"\n# c\n" + b1 + b2,                                      # lines skipped in front of the first run lie inside it
        HEADER + block(b"r", b"x", between=b"\n\n# two\ni x C 0 C 0\n\n") + b2 + b3,     # several lines between: behind the first
        HEADER + block(b"r", b"x", between=long_note) + b2,                 # a comment line of more than 4 KiB ends a block
        (HEADER + b1 + b2 + b3).replace(b"\n", b"\r\n"),                    # CRLF
        HEADER + b"a\n" + sline(b"r").replace(b"\n", b"   \t \n") + sline(b"x") + b"  \n" + b2,     # blanks behind the row
        HEADER + b1 + b"a\n" + sline(b"r") + sline(b"z"),                   # a last block without an ending line
        HEADER + b1 + b"a\n" + sline(b"r") + sline(b"z")[:-1],              # ... whose last row has no line feed either
        HEADER + b1 + b"a\n" + sline(b"r") + b"# the end",                  # an ending line without a final line feed
        HEADER + b"# nothing here\n\n",                                     # no block: the header's end is handed on
        HEADER[:-1],                                                        # a header without a line feed, alone
    ]
    for k, piece in enumerate(cases):
        got = check_piece(eng, piece, base=0, carry=123456789, shift=k % 16)
        assert got["next_offset"] != 123456789                             # skip == 0: the header line is always an anchor
        # the same lines behind the dummy line of a later piece: the first block takes the carry
        body = piece[piece.find(b"\n") + 1:] if b"\n" in piece else b""
        for base, carry in ((1000, 777), (1 << 40, (1 << 40) - 99)):       # 13-digit offsets
            later = check_piece(eng, b"#\n" + body, skip=2, base=base, carry=carry)
            if later["n_blocks"]:                                           # the piece's first s-line is group 0's first interval
                assert later["text"].split(b"}")[0].endswith(b'"offset":%d' % carry)
    got = check_piece(eng, b"#\n" + b"# a piece without a run\n\n", skip=2, base=5000, carry=4321)
    assert got["next_offset"] == 4321 and got["n_blocks"] == 0
    got = check_piece(eng, HEADER + b1 + b2, base=1 << 40)
    assert b'"offset":%d}' % ((1 << 40) + len(HEADER)) in got["text"] and got["next_offset"] == (1 << 40) + len(HEADER + b1 + b2)


def check_abi_numbers(eng):
    """start and align_size of 1 and 20 digits; their sum wraps"""
    vals = (0, 7, 10 ** 19, U64)
    rows = [(a, b) for a in vals for b in vals]
    piece = HEADER + b"".join(b"a\n" + sline(b"r", a, b, b"-" if k % 2 else b"+", U64) + sline(b"q", b, a) + b"\n" for k, (a, b) in enumerate(rows))
    got = check_piece(eng, piece, base=10 ** 12)
    assert b'{"start":18446744073709551615,"end":6,"strand":"-"' in got["text"]            # U64 + 7 wraps
    assert b'{"start":18446744073709551615,"end":18446744073709551614,' in got["text"]     # U64 + U64
    assert b'{"start":0,"end":0,' in got["text"] and b'"end":10000000000000000007,' in got["text"]
    assert int(got["names"][0]["size"]) == U64


def check_abi_errors(eng):
    dup_first = HEADER + block(b"r", b"x", b"x") + block(b"r", b"y")
    dup_later = HEADER + block(b"r", b"x") + block(b"r", b"y", b"z", b"y") + block(b"r", b"w", b"w")
    conflict = HEADER + block(b"r", b"x") + block(b"x", b"r")
    both_one_line = HEADER + block(b"r", b"x") + block(b"r", b"r")                         # its last line: a duplicate and a conflict
    dup_then_conflict = HEADER + block(b"r", b"x", b"x") + block(b"x", b"k")
    conflict_then_dup = HEADER + block(b"r", b"x") + block(b"x", b"k") + block(b"r", b"m", b"m")
    clean = HEADER + block(b"r", b"x") + block(b"r", b"x", b"y")
    want = {}
    for name, piece in (("dup_first", dup_first), ("dup_later", dup_later), ("conflict", conflict), ("both", both_one_line),
                        ("dup_then_conflict", dup_then_conflict), ("conflict_then_dup", conflict_then_dup), ("clean", clean)):
        got = check_piece(eng, piece)
        want[name] = (got["first_dup_line"], got["first_conflict_line"])
    # by hand: the header is line 0, a block's `a` line, then its rows
    assert want["dup_first"] == (4, None) and want["dup_later"] == (9, None) and want["conflict"] == (None, 6)
    assert want["both"] == (7, 7)
    assert want["dup_then_conflict"] == (4, 7) and want["conflict_then_dup"] == (12, 6) and want["clean"] == (None, None)
    # one block of 3 000 rows: the duplicate check does not depend on the block's size
    names = [b"n%d" % k for k in range(3000)]
    assert check_piece(eng, HEADER + block(*names))["first_dup_line"] is None
    names[2999] = names[5]
    assert check_piece(eng, HEADER + block(*names))["first_dup_line"] == 1 + 1 + 2999
    names[1500] = names[1499]
    assert check_piece(eng, HEADER + block(*names))["first_dup_line"] == 1 + 1 + 1500


def raw(eng, s, null=(), n_lines=None, n_bytes=None, skip=0, work=True):
    d_work = eng.empty(max(int(eng.lib.wga_maf_index_work_bytes(s.n_lines)), 16), np.uint8)
    host = {k: C.c_uint64(7) for k in ("names", "blocks", "slines", "text", "dup", "conflict", "next")}
    ptr = {k: C.byref(v) for k, v in host.items()}
    p = dict(d_text=s.d_text.ptr, d_lines=s.d_lines.ptr)
    for k in null:
        if k in p:
            p[k] = None
        else:
            ptr[k] = None
    rc = eng.lib.wga_maf_index(eng.ctx, p["d_text"], s.n_bytes if n_bytes is None else n_bytes, p["d_lines"],
                               s.n_lines if n_lines is None else n_lines, skip, 0, 55, d_work.ptr if work else None,
                               *(ptr[k] for k in ("names", "blocks", "slines", "text", "dup", "conflict", "next")), None, None)
    return rc, tuple(int(host[k].value) for k in ("names", "blocks", "slines", "text", "next"))


def check_abi_arguments(eng):
    s = Split(eng, HEADER + block(b"r", b"x") + block(b"r", b"y"))
    rc, (names, blocks, slines, text, nxt) = raw(eng, s)
    assert (rc, names, blocks, slines) == (0, 3, 2, 4) and text > 0 and nxt == s.n_bytes
    for k in ("names", "blocks", "slines", "text", "dup", "conflict", "next"):
        assert raw(eng, s, null=(k,))[0] == E_INVALID_ARG, k
        assert raw(eng, s, null=(k,), n_lines=0)[0] == E_INVALID_ARG, k                   # whatever the count
    assert raw(eng, s, work=False)[0] == E_INVALID_ARG and raw(eng, s, work=False, n_lines=0)[0] == E_INVALID_ARG
    for k in ("d_text", "d_lines"):
        assert raw(eng, s, null=(k,))[0] == E_INVALID_ARG, k
    assert raw(eng, s, n_bytes=0)[0] == E_INVALID_ARG
    assert raw(eng, s, n_lines=s.n_lines + 1)[0] == E_INVALID_ARG                         # not the text's line count
    assert raw(eng, s, skip=1)[0] == E_INVALID_ARG and raw(eng, s, skip=3)[0] == E_INVALID_ARG
    assert raw(eng, s, n_lines=0xFFFFFFFF)[0] == E_INVALID_ARG and raw(eng, s, n_bytes=0xFFFFFFF0)[0] == E_INVALID_ARG
    # n_lines == 0: zeros, the carry is handed on, nothing is written (Engine.maf_index checks the guards)
    assert raw(eng, s, n_lines=0, null=("d_text", "d_lines")) == (0, (0, 0, 0, 0, 55))
    got = eng.maf_index(None, 0, None, 0, skip=2, base=9, carry_offset=77)
    assert (got["n_names"], got["n_blocks"], got["n_slines"], got["text"], got["next_offset"]) == (0, 0, 0, b"", 77)
    # a table with a WGA_MAF_FALLBACK line is refused with a status of its own
    for bad in (b"s r 1 2 + 9\n", b"s r 1 x + 9 AC\n", b"s r\xc3\xa9 1 2 + 9 AC\n"):
        f = Split(eng, HEADER + block(b"r", b"x") + b"a\n" + bad + b"\n")
        assert 2 in f.d_lines.numpy()["status"][:f.n_lines]
        assert raw(eng, f)[0] == E_FALLBACK and eng.maf_index(*f.args()) is None
    # the fill call wants both arrays
    w = eng.empty(int(eng.lib.wga_maf_index_work_bytes(s.n_lines)), np.uint8)
    host = [C.c_uint64(0) for _ in range(7)]
    a = (eng.ctx, s.d_text.ptr, s.n_bytes, s.d_lines.ptr, s.n_lines, 0, 0, 0, w.ptr) + tuple(C.byref(v) for v in host)
    assert eng.lib.wga_maf_index(*a, None, None) == 0
    out, tab = eng.empty(int(host[3].value) + 16, np.uint8), eng.empty(48 * 4, np.uint8)
    assert eng.lib.wga_maf_index(*a, tab.ptr, None) == E_INVALID_ARG and eng.lib.wga_maf_index(*a, None, out.ptr) == E_INVALID_ARG
    assert eng.lib.wga_maf_index(*a, tab.ptr, out.ptr) == 0


def check_abi_reproducible(eng):
    """two calls give equal results, a workspace that another piece used before, and the fill writes what the count counted
    (Engine.maf_index checks that the counts stay and that nothing lies outside text_bytes)"""
    piece = counted_piece(700, seed=3)
    s = Split(eng, piece)
    work = eng.upload(np.full(int(eng.lib.wga_maf_index_work_bytes(s.n_lines)), 0x5A, dtype=np.uint8))
    a = eng.maf_index(*s.args(), work=work)
    other = Split(eng, interleaved_piece(17))
    eng.maf_index(*other.args(), work=work)
    b = eng.maf_index(*s.args(), work=work, out_shift=3)
    c = eng.maf_index(*s.args())
    for x in (b, c):
        assert x["text"] == a["text"] and x["names"].tobytes() == a["names"].tobytes()
        assert {k: v for k, v in x.items() if k not in ("text", "names")} == {k: v for k, v in a.items() if k not in ("text", "names")}
    assert len(a["text"]) == int(a["names"][-1]["text_off"]) and a["text"].count(b"{") == 700
    compare(piece, a, ref.piece_index(piece))


def check_abi_random(eng, seeds):
    for seed in seeds:
        blocks = mext.unique_names(random_blocks(seed, 25, 60))
        data = maf_text(blocks, noise=True, seed=seed)
        check_piece(eng, data, shift=seed % 16)
        cut = data.find(b"\na score", len(data) // 2) + 1                                 # the file in two pieces
        first = check_piece(eng, data[:cut])
        check_piece(eng, b"#\n" + data[cut:], skip=2, base=cut, carry=first["next_offset"])


# ---- the command -------------------------------------------------------------------------------------------------------------------
def index_three_ways(cli, path, env=None, want_error=None, device_phase=True):
    """the command under the device writer and under WGA_MAF_INDEX_WRITER=host, and the restatement: the same bytes in the index
    file, or the same message; under WGA_TIMING=1 each run names the path it took"""
    env = env or {}
    data = open(path, "rb").read()
    exp, exp_err = ref.index_text(data)
    out = []
    for e in (env, dict(env, **HOST_WRITER)):
        if os.path.exists(path + ".index"):
            os.remove(path + ".index")
        rc, _, msg, timing = m2p.timed(cli, ["maf-index", path], e)
        out.append((rc, msg, open(path + ".index", "rb").read() if rc == 0 else None, timing))
    (rc, msg, got, t_dev), (rc_h, msg_h, got_h, t_host) = out
    assert (rc, msg) == (rc_h, msg_h), (rc, rc_h, msg, msg_h)
    if exp_err:
        assert rc == 1 and exp_err in msg, (msg, exp_err)
        assert want_error is None or want_error in msg
        return None
    assert want_error is None and rc == 0, msg
    assert got == exp, mext_first_difference(got, exp)
    assert got_h == exp, mext_first_difference(got_h, exp)
    assert HOST_PHASE in t_host and DEVICE_PHASE not in t_host, t_host
    if device_phase:
        assert DEVICE_PHASE in t_dev, t_dev
    else:
        assert DEVICE_PHASE not in t_dev and HOST_PHASE in t_dev, t_dev
    return got, t_dev


def mext_first_difference(got, exp):
    k = next((i for i, (x, y) in enumerate(zip(got, exp)) if x != y), min(len(got), len(exp)))
    return len(got), len(exp), k, got[max(0, k - 80):k + 80], exp[max(0, k - 80):k + 80]


def check_cli_fixtures(cli, tmp_path):
    for name in ("test.maf", "test_chunk_l300.maf"):
        path = str(tmp_path / name)
        shutil.copy(os.path.join(GOLDEN, name), path)
        got, timing = index_three_ways(cli, path)
        assert HOST_PHASE not in timing                                                   # every piece went through the device
        for env in ({"WGA_CHUNK_BYTES": "200"}, {"WGA_CHUNK_BYTES": "4096"}):
            assert index_three_ways(cli, path, env=env)[0] == got


def check_cli_random(cli, tmp_path):
    """random files with noise lines, in one piece and in many: names that first appear in a later piece"""
    for seed in (71, 72):
        blocks = random_blocks(seed, 30, 120)
        blocks = [[(b"R%d" % (b % 4),) + rows[0][1:]] + [(b"q%d.%d" % (r, (b + r) % 5),) + row[1:] for r, row in enumerate(rows[1:])]
                  for b, rows in enumerate(blocks)]
        blocks[-1].append((b"late.name",) + blocks[-1][0][1:])
        path = str(tmp_path / ("r%d.maf" % seed))
        open(path, "wb").write(maf_text(blocks, noise=True, seed=seed))
        for env in ({}, {"WGA_CHUNK_BYTES": "200"}, {"WGA_CHUNK_BYTES": "4096"}):
            index_three_ways(cli, path, env=env)
        index_three_ways(cli, path, env={"WGA_MAF_READER": "host"}, device_phase=False)
        index_three_ways(cli, path, env={"WGA_MAF_READER": "host", "WGA_CHUNK_BYTES": "4096"}, device_phase=False)


def error_files():
    filler = b"".join(block(b"r", b"f%d" % k, start=1000 * k) for k in range(30))
    return {
        "conflict_far.maf": HEADER + block(b"r", b"x") + filler + block(b"x", b"k"),          # x: a query, pieces later a reference
        "dup_far.maf": HEADER + block(b"r", b"x") + filler + block(b"r", b"y", b"y"),
        "conflict_then_dup.maf": HEADER + block(b"r", b"x") + filler + block(b"x", b"k") + filler + block(b"r", b"m", b"m"),
        "dup_then_conflict.maf": HEADER + block(b"r", b"x") + filler + block(b"r", b"m", b"m") + filler + block(b"x", b"k"),
        "both_one_line.maf": HEADER + block(b"r", b"x") + filler + block(b"r", b"r"),
        "empty.maf": HEADER + b"\n# nothing\n",
    }


ERROR_FILES = tuple(error_files())


def check_cli_errors_across_pieces(cli, tmp_path, name):
    """a conflict and a duplicate that only show across pieces, and which of two errors is reported"""
    files = error_files()
    path = str(tmp_path / name)
    open(path, "wb").write(files[name])
    for env in ({}, {"WGA_CHUNK_BYTES": "200"}, {"WGA_CHUNK_BYTES": "4096"}):
        assert index_three_ways(cli, path, env=env) is None, (name, env)
    assert "Same sequence" in ref.index_text(files["conflict_then_dup.maf"])[1]
    assert "Duplicate name `m`" in ref.index_text(files["dup_then_conflict.maf"])[1]
    assert "Duplicate name `r`" in ref.index_text(files["both_one_line.maf"])[1]            # the duplicate goes first (index.rs:32-56)


def check_cli_fallback_piece(cli, tmp_path):
    """a name with a non-ASCII byte makes its piece the host reader's, between two device pieces: both loops append to the same
    entries and the offset walk takes over and hands back"""
    front = b"".join(block(b"r", b"x%d" % (k % 3), start=100 * k) for k in range(12))
    odd = block(b"r", b"caf\xc3\xa9", b"x1", start=77) + block(b"r", b"x2", start=99)
    back = b"".join(block(b"r", b"x%d" % (k % 4), b"late%d" % (k % 2), start=100 * k) for k in range(12))
    path = str(tmp_path / "fb.maf")
    open(path, "wb").write(HEADER + front + odd + back + odd + back)
    got, timing = index_three_ways(cli, path, env={"WGA_CHUNK_BYTES": "300"})
    assert DEVICE_PHASE in timing and HOST_PHASE in timing and b'"caf\xc3\xa9":' in got
    got_one, timing = index_three_ways(cli, path, device_phase=False)                       # one piece: all of it the host reader's
    assert got_one == got


def check_cli_loop_closure(cli, tmp_path):
    """the error cases and -o of maf_ext_cases, and maf-ext and call reading the index the device wrote"""
    mext.check_index_errors_and_output(cli, tmp_path)
    mext.check_index_then_call(cli, tmp_path)
    mext.check_literal(cli, tmp_path)
    good = b"a\ns na\"me\\z 4 2 + 9 AC\ns y 3 2 - 9 A-C\ns c\x01t\x1fl 0 1 + 9 --A\n\n"
    path = str(tmp_path / "esc.maf")
    open(path, "wb").write(HEADER + good)
    got, _ = index_three_ways(cli, path)
    assert got.startswith(b'{"na\\"me\\\\z":{"ivls":[{"start":4,"end":6,"strand":"+","offset":16}],"size":9,"isref":true},')
    assert b'"c\\u0001t\\u001fl":' in got


def check_cli_timing(cli, tmp_path):
    path = str(tmp_path / "t.maf")
    shutil.copy(os.path.join(GOLDEN, "test.maf"), path)
    rc, _, msg, timing = m2p.timed(cli, ["maf-index", path], {})
    assert rc == 0 and DEVICE_PHASE in timing and HOST_PHASE not in timing, (msg, timing)
    rc, _, msg, timing = m2p.timed(cli, ["maf-index", path], HOST_WRITER)
    assert rc == 0 and HOST_PHASE in timing and DEVICE_PHASE not in timing, (msg, timing)
