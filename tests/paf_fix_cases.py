"""`validate --fix` on the device (K29): the C-ABI entries (Engine.paf_split -> Engine.paf_fix_plan -> tokeniser -> K1 ->
Engine.paf_fix) and the `wgatools validate --fix` command with its device path against its host writer.  The expectation is
paf_fix_ref, the restatement from the file's bytes.  Imported by test_emu_paf_fix.py (emulator build, CPU) and
test_gpu_paf_fix.py (the product on a GPU); each provides the `cli` and `eng` fixtures."""
import os
import random
import re

import numpy as np

import paf_fix_ref as ref
from paf_filter_cases import GOLDEN, paf_line, random_file, run, split, with_field, write  # noqa: F401
from wgatools_amd.engine import PAF_FIX_TILE, PAF_OK, Batch

U64 = (1 << 64) - 1
T = PAF_FIX_TILE


# ---- texts ---------------------------------------------------------------------------------------------------------------------
def cg_of_bytes(n):
    """a CIGAR text of exactly n >= 2 bytes, all `=` ops of one or eleven bases"""
    assert n >= 2
    return b"11=" + b"1=" * ((n - 3) // 2) if n % 2 else b"1=" * (n // 2)


def cg_sums_of_bytes(n):
    """what paf_fix_ref.cigar_sums gives for cg_of_bytes(n), without reading it"""
    k = 11 + (n - 3) // 2 if n % 2 else n // 2
    return k, k


def fix_line(qs=0, qe=None, ts=10, te=None, cg=b"10=", tags_before=(b"tp:A:P",), tags_after=(), **kw):
    """one record; an end that is not given is the one the CIGAR asks for"""
    if qe is None or te is None:
        dq, dt = ref.cigar_sums(cg)
        qe = (qs + dq) & U64 if qe is None else qe
        te = (ts + dt) & U64 if te is None else te
    return paf_line(qs=qs, qe=qe, ts=ts, te=te, tags=tuple(tags_before) + (b"cg:Z:" + cg,) + tuple(tags_after), **kw)


def fix_line_of_len(n, **kw):
    """a record line of exactly n bytes, its newline included: the CIGAR takes up the slack.  A wrong end must be given as an
    offset from the right one (qe_off / te_off), since the right one moves with the CIGAR."""
    qe_off, te_off = kw.pop("qe_off", 0), kw.pop("te_off", 0)
    cg_bytes = max(2, n - len(fix_line(cg=b"", qe=0, te=0, **kw)))
    for _ in range(12):                                                         # the ends' digits move the length a little
        dq, dt = cg_sums_of_bytes(cg_bytes)
        ln = fix_line(cg=cg_of_bytes(cg_bytes), qe=(kw.get("qs", 0) + dq + qe_off) & U64, te=(kw.get("ts", 10) + dt + te_off) & U64, **kw)
        if len(ln) == n:
            return ln
        cg_bytes += n - len(ln)
        assert cg_bytes >= 2, n
    raise AssertionError(n)


def fix_field(col, value, **kw):
    """a record whose column `col` holds `value` as it is (`007`, `+5`)"""
    f = fix_line(**kw).rstrip(b"\n").split(b"\t")
    f[col] = value
    return b"\t".join(f) + b"\n"


def random_fix_file(seed, **kw):
    """paf_filter_cases.random_file with a cg:Z: tag on every record (in front of, between and behind the other tags, both
    strands, CIGARs from 5 bytes to 40 KB); every second record or so gets the ends its CIGAR asks for"""
    kw.setdefault("cg_bytes", (5, 100, 9000, 40000))
    data = random_file(seed, **kw)
    rng = random.Random(seed + 1000)
    out = []
    for ln in data.split(b"\n"):
        if ln and not ln.startswith(b"#"):                                      # random_file may end a cut CIGAR with a bare `=`
            ln = b"\t".join(re.sub(rb"([=XIDM])=$", rb"\1", t) if t.startswith(b"cg:Z:") else t for t in ln.split(b"\t"))
        if ln and not ln.startswith(b"#") and rng.random() < 0.5:
            f = ln.split(b"\t")
            dq, dt = ref.cigar_sums(ref.cigar_of(f))
            which = rng.randrange(3)                                           # both right, only the query's, only the target's
            if which != 2:
                f[3] = b"%d" % (int(f[2]) + dq)
            if which != 1:
                f[8] = b"%d" % (int(f[7]) + dt)
            ln = b"\t".join(f)
        out.append(ln)
    return b"\n".join(out)


# ---- ABI level -----------------------------------------------------------------------------------------------------------------
def device_fix(eng, data, want=(True, True, True)):
    """split, plan, tokenise, K1, fix.  Returns (rows, qlist, tlist, sizes), or the first untaken line"""
    d_text, n, d_lines = split(eng, data)
    nr, bad, beg, end = eng.paf_fix_plan(d_text, len(data), d_lines, n)     # the words around the spans are checked in there
    if bad is not None:
        assert nr == 0
        return bad
    counts = None
    if nr:
        cnt, err = eng.cigar_tokenise_spans(nr, d_text, beg, end)
        off = eng.exclusive_scan_u64(nr, cnt)
        tot = int(off.numpy()[-1])
        ops = eng.empty(tot + 4, np.uint32).fill(0)
        eng.cigar_tokenise_spans(nr, d_text, beg, end, op_cnt=cnt, err=err, ops=ops, op_off=off)
        assert not err.numpy()["err"].any()
        lines = d_lines.numpy()[:n]
        strand = lines["strand_neg"][lines["status"] == PAF_OK]                 # '-' records count in the inv_* slots
        assert len(strand) == nr
        batch = Batch(ops, off, eng.upload(np.concatenate([strand, np.zeros(16, np.uint8)])), nr, tot)
        counts, diag, _ = eng.cigar_stat(batch, want_tiles=False)
        assert (diag.numpy()["bad_op_idx"] == U64).all()
        if strand.any():
            c = counts.numpy()[:nr]
            neg = strand != 0
            assert not (c["ins_bp"][neg].any() or c["del_bp"][neg].any() or c["inv_ins_bp"][~neg].any() or c["inv_del_bp"][~neg].any())
    return eng.paf_fix(d_text, len(data), d_lines, n, counts, nr, want)    # ... and the guards around the three texts in there


def check(eng, data, want=(True, True, True)):
    """a taken text: the device's three texts and its counts are the restatement's"""
    got = device_fix(eng, data, want)
    assert not isinstance(got, int), (got, data[:200])
    rows, ql, tl, sizes = got
    e_rows, e_ql, e_tl, n, nq, nt = ref.fix(data)
    assert sizes == {"rows_bytes": len(e_rows), "qlist_bytes": len(e_ql), "tlist_bytes": len(e_tl), "n_records": n, "n_q_bad": nq,
                     "n_t_bad": nt}, (sizes, data[:200])
    for g, e, w in ((rows, e_rows, want[0]), (ql, e_ql, want[1]), (tl, e_tl, want[2])):
        assert (g == e) if w else (g is None), (len(e), data[:200])
    return e_rows, e_ql, e_tl


def check_untaken(eng, data, line):
    assert device_fix(eng, data) == line, (line, data[:200])


def check_abi_digit_counts(eng):
    near = (1 << 64) - 3                                                        # a start that wraps with `5=`: the end is 2
    recs = [fix_line(q=b"a", qs=0, qe=9, cg=b"10="),                            # 9 -> 10
            fix_line(q=b"b", qs=0, qe=99, cg=b"100="),                          # 99 -> 100
            fix_line(q=b"c", qs=0, qe=100, cg=b"99="),                          # 100 -> 99
            fix_line(q=b"d", qs=near - 2, qe=10, cg=b"5="),                     # 10 -> 0, wrapping
            fix_line(q=b"e", qs=(1 << 64) - 10, qe=7, cg=b"5="),                # 1 -> 20 digits
            fix_line(q=b"f", qs=near, qe=U64, cg=b"5="),                        # 20 digits -> 1, wrapping
            fix_line(q=b"g", qs=near, qe=2, cg=b"5="),                          # the wrapped end is the old one: not bad
            fix_line(q=b"h", ts=0, te=9, cg=b"10="),                            # the same on column 9
            fix_line(q=b"i", ts=0, te=100, cg=b"99="),
            fix_line(q=b"j", ts=near - 2, te=10, cg=b"5="),
            fix_line(q=b"k", ts=(1 << 64) - 10, te=7, cg=b"5="),
            fix_line(q=b"l", ts=near, te=U64, cg=b"5="),
            fix_line(q=b"m", ts=near, te=2, cg=b"5="),
            fix_line(q=b"n", qe=1, te=1, cg=b"4=3I2D1X"),                       # both wrong
            fix_line(q=b"o", qe=1, cg=b"4=3I2D1X"),                             # only column 4
            fix_line(q=b"p", te=1, cg=b"4=3I2D1X"),                             # only column 9
            fix_line(q=b"r", cg=b"4=3I2D1X"),                                   # neither
            fix_line(q=b"s", strand=b"-", qe=1, te=1, cg=b"4M3I2D1X")]          # '-': the inv_* slots
    data = b"".join(recs)
    rows, ql, tl = check(eng, data)
    assert rows.split(b"\n")[3].split(b"\t")[3] == b"0" and rows.split(b"\n")[4].split(b"\t")[3] == b"%d" % ((1 << 64) - 5)
    assert rows.split(b"\n")[5].split(b"\t")[3] == b"2" and rows.split(b"\n")[6] == recs[6][:-1]
    assert ql.count(b"\n") == 9 and tl.count(b"\n") == 8
    for ln in recs:                                                             # ... and every record alone
        check(eng, ln)
    for a, b in ((0, 6), (6, 13), (13, 18)):
        check(eng, b"".join(reversed(recs[a:b])))


def place(build_target, byte_at, pos, lead=b""):
    """lead, a filler record and a target record such that the target's output byte number byte_at(row) lands at `pos` of the
    rows; returns the file"""
    target = build_target()
    row = ref.fix(target)[0]
    lead_out = len(ref.fix(lead)[0]) if lead else 0
    fill = pos - byte_at(row) - lead_out
    data = lead + fix_line_of_len(fill, q=b"fill") + target
    rows = ref.fix(data)[0]
    assert rows.endswith(row) and len(rows) - len(row) + byte_at(row) == pos
    return data


def field_start(col):
    return lambda row: len(b"\t".join(row.split(b"\t")[:col])) + 1


def field_last(col):
    return lambda row: len(b"\t".join(row.split(b"\t")[:col + 1])) - 1


def field_tab(col):
    return lambda row: len(b"\t".join(row.split(b"\t")[:col + 1]))


def check_abi_tile_and_group_edges(eng):
    targets = (lambda: fix_line(q=b"tq", qs=123, qe=99, cg=b"5000=7I", tags_after=(b"zz:Z:after",)),                 # column 4: 99 -> 5130
               lambda: fix_line(q=b"tt", ts=10 ** 6, te=1234567, cg=b"20=3D", tags_after=(b"zz:Z:after",)),         # column 9: shorter
               lambda: fix_line(q=b"tb", qs=5, qe=6, ts=7, te=8, cg=b"300=", tags_before=()))                        # both
    lead = fix_line(q=b"lead", qe=1, te=10 ** 9, cg=b"77=")                     # rows in front that are not where their lines were
    for build, col in ((targets[0], 3), (targets[1], 8), (targets[2], 3), (targets[2], 8)):
        for at in (field_start(col), field_last(col), field_tab(col), lambda row: len(row) - 1):
            for border in (T, T + 160, 2 * T):                                  # a tile's edge, a 16-byte group's, the next tile's
                for side in (-1, 0):
                    check(eng, place(build, at, border + side, lead if border != T else b"") + fix_line(q=b"behind", qe=3))
    short = [fix_line(q=b"s%d" % k, qe=(k % 3), te=(k % 2) * 7, cg=b"%d=" % (k + 1)) for k in range(8)]
    for shift in range(0, 48, 5):                                               # short records straddle the tile's edge byte by byte
        check(eng, fix_line_of_len(T - 30 - shift) + b"".join(short))
    long_line = fix_line_of_len(7 * T // 2 + 3, q=b"long", qe_off=5, te_off=-3)  # 3.5 tiles between 60-byte lines
    data = b"".join(short[:4]) + long_line + b"".join(short[4:])
    rows, ql, tl = check(eng, data)
    assert len(rows) > 3 * T and b"long:" in ql
    check(eng, fix_line_of_len(7 * T // 2 + 3, q=b"long"))                      # ... the same line alone, nothing to fix
    many = b"".join(fix_line(q=b"m%d" % k, qe=(k % 5) * 30, te=40, cg=b"%d=" % (k % 4 * 10 + 30)) for k in range(700))
    assert len(many) > 4 * T                                                    # tiles of ~150 short records
    rows, ql, tl = check(eng, many)
    assert check(eng, many[:-1])[0] == rows                                     # an unterminated last line gains its newline
    check(eng, many[:-1] + b"\tzz:Z:tail")
    inter = b"#head\n\n" + b"".join(ln + (b"\n" if k % 3 == 0 else b"#c%d\n" % k if k % 3 == 1 else b"") for k, ln in enumerate(short * 40))
    assert check(eng, inter)[0] == ref.fix(b"".join(short * 40))[0]             # `#` and blank lines first and between
    check(eng, inter + b"#no newline at the end")                               # ... and last
    check(eng, inter + b"\n\n")
    assert device_fix(eng, b"\n\n#x\n")[:3] == (b"", b"", b"")                  # only SKIP lines
    assert device_fix(eng, b"#x")[3]["n_records"] == 0
    assert device_fix(eng, b"")[:3] == (b"", b"", b"")                          # n_lines == 0
    check(eng, fix_line(qe=1))                                                  # one record
    check(eng, fix_line(qe=1, end=b""))
    for n in (255, 256, 257, 1024, 1025):                                       # the line passes' and the scans' blocks
        check(eng, b"".join(fix_line(q=b"n%d" % k, qe=k % 7, cg=b"%d=" % (k % 7 or 3)) for k in range(n)))


def check_abi_lists(eng):
    good = b"".join(fix_line(q=b"g%d" % k, cg=b"%d=2I" % (k + 1)) for k in range(300))
    rows, ql, tl = check(eng, good)                                             # none bad
    assert rows == good and ql == b"" and tl == b""
    assert check(eng, good, want=(True, False, False))[0] == good               # ... the lists' pointers may be NULL
    bad = b"".join(fix_line(q=b"b%d" % k, t=b"t%d" % (k % 7), qe=0, te=1, cg=b"%d=2I" % (k + 1)) for k in range(300))
    rows, ql, tl = check(eng, bad)                                              # all bad
    assert ql.count(b"\n") == 300 and tl.count(b"\n") == 300
    check(eng, bad, want=(False, True, True))                                   # ... each text on its own
    check(eng, bad, want=(False, True, False))
    check(eng, bad, want=(False, False, True))
    check(eng, bad, want=(True, False, False))
    name = b"scaffold_" + b"x" * 3000
    longn = fix_line(q=name, t=name[::-1], qe=1, te=2) + fix_line(q=b"q", t=name, te=3) + fix_line(q=name, t=b"t", qe=4)
    rows, ql, tl = check(eng, longn)                                            # long names
    assert ql == name + b":0-1\n" + name + b":0-4\n"
    same = fix_line(q=b"same", t=b"same", qs=1, qe=2, ts=3, te=4) * 3           # the same name bad for query and target
    rows, ql, tl = check(eng, same)
    assert ql == b"same:1-2\n" * 3 and tl == b"same:3-4\n" * 3


def untaken_lines():
    hi = b"\xc3\xa9"
    bad = [fix_line(q=b'"q"'), fix_line(end=b"\r\n"), fix_line(q=b"caf" + hi), fix_line(tags_after=(b"zz:Z:" + hi,)),
           paf_line(tags=(b"tp:A:P",)),                                         # a record without cg:Z:
           paf_line(tags=(b"cs:Z::10",)),                                       # cs:Z: standing in
           b"\t".join(fix_line().split(b"\t")[:11]) + b"\n"]                    # 11 fields
    return bad + [fix_field(col, v) for col in ref.NUM_COLS for v in (b"007", b"+5")]


def check_abi_untaken(eng):
    good = fix_line(q=b"g", qe=1)
    for ln in untaken_lines():
        check_untaken(eng, good * 3 + ln + good, 3)
    check_untaken(eng, good + b"#comm\xc3\xa9nt\n" + good, 1)                   # a byte >= 0x80 on a SKIP line
    check_untaken(eng, good * 2 + paf_line() + good * 300 + with_field(2, b"+1"), 2)      # the lowest, across blocks
    check_untaken(eng, good * 300 + with_field(2, b"+1") + paf_line(), 300)
    check_untaken(eng, good * 5 + paf_line(end=b""), 5)                         # in an unterminated last line
    for v in (b"0", b"10"):                                                     # canonical numbers are taken
        for col in (1, 6, 9, 10, 11):
            check(eng, good + fix_field(col, v))


def check_abi_random_files(eng, seeds=range(12)):
    for seed in seeds:
        data = random_fix_file(seed, end=seed % 3 != 0)
        assert 10000 < len(data) < (1 << 23)
        rows, ql, tl = check(eng, data)
        n = len(ref.records(data))
        assert 0 < ql.count(b"\n") < n and 0 < tl.count(b"\n") < n and rows != data


# ---- the restatement itself (CPU) ----------------------------------------------------------------------------------------------
def check_reference_properties():
    rows = [b"q1\t100\t10\t30\t+\tt1\t200\t5\t25\t0\t0\t60\tcg:Z:10=2I8=\tNM:i:2", b"q2\t100\t0\t20\t-\tt1\t200\t0\t20\t0\t0\t60\tcg:Z:10=3D7=",
            b"q3\t50\t0\t12\t+\tt2\t60\t1\t13\t0\t0\t0\tcg:Z:5=1X6="]
    data = b"\n".join(rows) + b"\n"                                            # the plain rows of cli_cases.test_validate_report_and_fix
    want = [rows[0].replace(b"\t5\t25\t", b"\t5\t23\t"), rows[1].replace(b"\t0\t20\t-", b"\t0\t17\t-"), rows[2]]
    assert ref.fix(data) == (b"\n".join(want) + b"\n", b"q2:0-20\n", b"t1:5-25\n", 3, 1, 1)
    assert ref.report(data) == (b"Total records: 3\nQuery invalid records: 1\nTarget invalid records: 1\nQuery invalid list:\nq2:0-20\n"
                                b"Target invalid list:\nt1:5-25\n\n")
    assert ref.fix(data[:-1]) == ref.fix(data) and ref.fix(b"#c\n\n" + data) == ref.fix(data)
    assert ref.cigar_sums(b"3M2=1X4I5D") == (10, 11)
    for n in range(2, 40):
        assert len(cg_of_bytes(n)) == n and ref.cigar_sums(cg_of_bytes(n)) == cg_sums_of_bytes(n)
    for n in (80, 81, T, 3 * T + 5):
        assert len(fix_line_of_len(n)) == n and ref.fix(fix_line_of_len(n))[1:] == (b"", b"", 1, 0, 0)
        assert ref.fix(fix_line_of_len(n, qe_off=1, te_off=-1))[3:] == (1, 1, 1)


# ---- command level -------------------------------------------------------------------------------------------------------------
HOST_WRITER = {"WGA_VALIDATE_WRITER": "host"}
HOST_READER = {"WGA_PAF_READER": "host"}
CHUNK = {"WGA_CHUNK_BYTES": "4000"}


def paths_of(cli, path, env=None):
    rc, out, err = run(cli, "__validate_fix_path", path, env=env)
    assert rc == 0, err
    return out.decode().split()


def cli_random_file(seed, end=True):
    return random_fix_file(seed, n_lines=60, cg_bytes=(5, 100, 9000), end=end)


def four_piece_file(bad=None, where=2):
    """four pieces under WGA_CHUNK_BYTES=4000 (a piece ends behind the first line end at or after 4000 bytes); `bad` replaces a
    line in the middle of piece `where`"""
    piece = [[fix_line(q=b"p%dq%d" % (p, k % 3), t=b"t%d" % (k % 2), qs=k, qe=(None if k % 3 else k), te=(None if k % 4 else 3 * k + p),
                       cg=b"%d=%dI%dD" % (k + 1, p + 1, k % 5 + 1)) for k in range(60)] for p in range(4)]
    for p in piece:
        assert 3000 < len(b"".join(p)) < 4000
    if bad is not None:
        piece[where][30] = bad
    return b"".join(b"".join(p) + fix_line_of_len(1200, q=b"fill", te_off=1) for p in piece)


PATH_PARTS = ("plain", "untaken", "pieces")


def check_path_selection(cli, tmp_path, part):
    if part == "plain":
        path = write(tmp_path, "r0.paf", cli_random_file(0))
        assert paths_of(cli, path) == ["device"]
        assert paths_of(cli, path, env=HOST_WRITER) == ["host"]
        assert paths_of(cli, path, env=HOST_READER) == ["host"]
        many = paths_of(cli, path, env=CHUNK)
        assert len(many) > 5 and set(many) == {"device"}
        assert paths_of(cli, write(tmp_path, "empty.paf", b"")) == []
    elif part == "untaken":
        # every untaken kind in a piece of its own between taken pieces: under WGA_CHUNK_BYTES=300 a piece ends behind the first
        # line end at or after 300 bytes, so a short line and a filler of 300 bytes are one piece
        good, fill = fix_line(qe=1), fix_line_of_len(300, q=b"fill")
        kinds = [ln for ln in untaken_lines() if b'"' not in ln]
        assert len(kinds) == 24 and all(len(ln) < 300 for ln in kinds)
        data = b"".join(good + fill + ln + fill for ln in kinds) + good
        got = paths_of(cli, write(tmp_path, "kinds.paf", data), env={"WGA_CHUNK_BYTES": "300"})
        assert got == ["device", "host"] * len(kinds) + ["device"]
        quote = [ln for ln in untaken_lines() if b'"' in ln]                        # the piece reader does not cut a text with a quote
        assert len(quote) == 1 and paths_of(cli, write(tmp_path, "quote.paf", good * 3 + quote[0] + good)) == ["host"]
    else:
        assert paths_of(cli, write(tmp_path, "four.paf", four_piece_file()), env=CHUNK) == ["device"] * 4
        seven = write(tmp_path, "four7.paf", four_piece_file(fix_field(7, b"007")))
        assert paths_of(cli, seven, env=CHUNK) == ["device", "device", "host", "device"]
        assert paths_of(cli, seven, env=dict(CHUNK, **HOST_WRITER)) == ["host"] * 4
        assert paths_of(cli, seven, env=dict(CHUNK, **HOST_READER)) == ["host"] * 4


def byte_files():
    files = {"r0": cli_random_file(0), "r1": cli_random_file(1, end=False), "four": four_piece_file(),
             "small": random_fix_file(5, n_lines=40, cg_bytes=(5, 100))}
    gold = open(GOLDEN, "rb").read()
    if all(any(t.startswith(b"cg:Z:") for t in f[12:]) for f in ref.records(gold)):
        files["gold"] = gold
    return files


BYTE_FILES = ("r0", "r1", "four", "small", "gold")


def validate_fix(cli, tmp_path, path, env=None, tag="x"):
    """(rc, report, fixed file, stderr lines) of `validate --fix FILE`"""
    fixed = str(tmp_path / ("fixed_%s.paf" % tag))
    if os.path.exists(fixed):
        os.remove(fixed)
    rc, out, err = run(cli, "validate", path, "--fix", fixed, env=env)
    return rc, out, (open(fixed, "rb").read() if os.path.exists(fixed) else None), err


def check_bytes(cli, tmp_path, name):
    """device path == host writer == the restatement: report and fixed file, `-f FILE` and `-f -`, whole and in pieces"""
    files = byte_files()
    if name not in files:
        assert name == "gold"                                                   # the golden file's records carry no cg:Z:
        return
    data = files[name]
    path = write(tmp_path, name + ".paf", data)
    want = (0, ref.report(data), ref.fix(data)[0], [])
    assert want[2] and (want[2] != data or name == "gold")                      # the golden file's ends are right
    small = {"WGA_CHUNK_BYTES": "64" if name in ("small", "gold") else "1500"}
    assert len(paths_of(cli, path, env=small)) >= 5 or name == "gold"           # two records: two pieces
    for k, env in enumerate(({}, CHUNK, small)):
        assert validate_fix(cli, tmp_path, path, env, "d%d" % k) == want, (name, env)
        assert validate_fix(cli, tmp_path, path, dict(env, **HOST_WRITER), "h%d" % k) == want, (name, env)
        assert run(cli, "validate", path, "-f", "-", env=env) == (0, want[1] + want[2], []), (name, env)
        if k == 0:
            assert run(cli, "validate", path, "-f", "-", env=HOST_WRITER) == (0, want[1] + want[2], []), name
    assert validate_fix(cli, tmp_path, path, HOST_READER, "r") == want
    assert run(cli, "validate", path) == (0, want[1], [])                       # without --fix: today's path, the same report
    assert run(cli, "vf", "-f", "-", stdin=data, env=CHUNK) == (0, want[1] + want[2], [])


def check_alternation(cli, tmp_path):
    """pieces that alternate taken / untaken: lists and rows in input order across the pieces"""
    for bad, where in ((fix_field(7, b"007", qe=1), (1, 3)), (fix_field(2, b"+5", te=1), (0, 2)), (fix_line(q=b'"quoted"', qe=1, te=2), (1, 3))):
        piece = [b"".join(fix_line(q=b"p%dq%d" % (p, k % 3), t=b"t%d" % (k % 2), qs=k, qe=(None if k % 3 else k), te=(None if k % 4 else p),
                                   cg=b"%d=%dI" % (k + 1, p + 1)) for k in range(60)) for p in range(4)]
        assert all(3000 < len(p) < 4000 for p in piece)
        rows = [p if k not in where else p[:1500].rsplit(b"\n", 1)[0] + b"\n" + bad + p[1500:].split(b"\n", 1)[1] for k, p in enumerate(piece)]
        data = b"".join(r + fix_line_of_len(1200, q=b"fill", qe_off=2) for r in rows)
        path = write(tmp_path, "alt.paf", data)
        if b'"' in bad:                                                         # the piece reader does not cut a text with a quote in it
            assert paths_of(cli, path, env=CHUNK) == ["host"]
        else:
            assert paths_of(cli, path, env=CHUNK) == ["host" if k in where else "device" for k in range(4)]
        got = validate_fix(cli, tmp_path, path, CHUNK, "alt")
        assert got == validate_fix(cli, tmp_path, path, dict(CHUNK, **HOST_WRITER), "alth") and got[0] == 0 and got[3] == []
        assert got == validate_fix(cli, tmp_path, path, {}, "altw")
        if b'"' not in bad:                                                     # the restatement reads plain text only
            assert got[1:3] == (ref.report(data), ref.fix(data)[0])
        assert run(cli, "validate", path, "-f", "-", env=CHUNK) == (0, got[1] + got[2], [])


def check_errors(cli, tmp_path):
    # an invalid op in the third of four pieces: exit 1, nothing written, the reference's panic text
    path = write(tmp_path, "op.paf", four_piece_file(fix_line(q=b"q9", qe=1, te=1, cg=b"3=") .replace(b"cg:Z:3=", b"cg:Z:3=2N")))
    assert paths_of(cli, path, env=CHUNK)[:2] == ["device", "device"]
    for env in (CHUNK, {}):
        got = validate_fix(cli, tmp_path, path, env, "op")
        assert got == validate_fix(cli, tmp_path, path, dict(env, **HOST_WRITER), "oph")
        assert got[0] == 1 and got[1] == b"" and not got[2] and got[3][-1].endswith("CIGAR OP `N` invalid"), got
        assert run(cli, "validate", path, "-f", "-", env=env)[:2] == (1, b"")
    # a broken line in a later piece: the reader's error text, with the line and byte numbers of the host writer's run
    short = b"\t".join(fix_line().split(b"\t")[:11]) + b"\n"
    path = write(tmp_path, "short.paf", four_piece_file(short))
    assert paths_of(cli, path, env=CHUNK)[:2] == ["device", "device"]
    n_before = four_piece_file(short).index(short)
    n_recs = four_piece_file(short)[:n_before].count(b"\n")
    for env in (CHUNK, {}):
        got = validate_fix(cli, tmp_path, path, env, "sh")
        assert got == validate_fix(cli, tmp_path, path, dict(env, **HOST_WRITER), "shh")
        assert got[0] == 1 and got[1] == b"" and not got[2], got
        assert "invalid length 11" in got[3][-1] and "record %d (line: %d, byte: %d)" % (n_recs, n_recs + 1, n_before) in got[3][-1], got[3]
