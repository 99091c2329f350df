"""`chunk` cases: the C-ABI entry (Engine.maf_chunk, K20) window by window and the `wgatools chunk` command line, against the
restatement in maf_chunk_ref.py.  Imported by test_emu_maf_chunk.py (emulator build, CPU) and test_gpu_maf_chunk.py (the
product on a GPU); each provides the `cli` and `eng` fixtures."""
import gzip
import os
import random
import subprocess

import numpy as np
import pytest

import maf_chunk_ref as ref
from helpers import GOLDEN
from wgatools_amd.engine import MAF_CHUNK_BLOCK_DTYPE, MAF_CHUNK_ROW_DTYPE


def run(cli, *args, env=None, stdin=None):
    e = dict(os.environ, **(env or {}))
    r = subprocess.run([cli] + list(args), stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=e, input=stdin)
    return r.returncode, r.stdout, r.stderr.decode()


# ---- random MAF ------------------------------------------------------------------------------------------------------------
def _row_text(rng, n):
    out = bytearray()
    while len(out) < n:
        run_len = rng.randint(1, 12)
        ch = b"-" if rng.random() < 0.3 else bytes([rng.choice(b"ACGTacgtN")])
        out += ch * run_len
    return bytes(out[:n])


def random_blocks(seed, n_blocks, max_cols, max_rows=6, longer=True, gappy=True):
    """blocks of 1 .. max_rows rows: gaps in runs, '-' strands, all-gap stretches, size fields that disagree with the text,
    rows longer than the first (their columns past the block's end are dropped)"""
    rng = random.Random(seed)
    blocks = []
    for b in range(n_blocks):
        cols = rng.randint(1, max_cols)
        rows = []
        for r in range(rng.randint(1, max_rows)):
            n = cols + (rng.randint(1, 40) if longer and r and rng.random() < 0.2 else 0)
            seq = _row_text(rng, n) if gappy else bytes(rng.choice(b"ACGT") for _ in range(n))
            if gappy and rng.random() < 0.2:
                a = rng.randint(0, n - 1)
                seq = seq[:a] + b"-" * min(n - a, rng.randint(1, 80)) + seq[a + rng.randint(1, 80):]
                seq = seq[:n].ljust(n, b"-")
            start = rng.randint(0, 10 ** rng.randint(1, 12))
            size = n - seq.count(b"-") + (rng.randint(1, 5) if rng.random() < 0.2 else 0)
            rows.append((b"chr%d.%d" % (b, r) if rng.random() < 0.5 else b"sp%d" % r, start, size,
                         b"-" if rng.random() < 0.4 else b"+", start + size + rng.randint(0, 10 ** 6), seq))
        blocks.append(rows)
    return blocks


def maf_text(blocks, noise=True, seed=0):
    rng = random.Random(seed)
    out = [b"##maf version=1 scoring=x\n"]
    for rows in blocks:
        out.append(b"a score=%d\n" % rng.randint(0, 99999))
        for (name, start, size, strand, src, seq) in rows:
            out.append(b"s %s %d %d %s %d %s\n" % (name, start, size, strand, src, seq))
        if noise:
            out.append(rng.choice([b"i x C 0 C 0\n", b"e y 1 2 + 3 I\n", b"q z 999\n", b"# note\n", b""]))
        out.append(b"\n")
    return b"".join(out)


def expected(blocks, L):
    text, panic = ref.chunk_text(blocks, L)
    return ref.header(L) + text, panic


# ---- ABI level -------------------------------------------------------------------------------------------------------------
def abi_chunk(eng, blocks, L, window_records):
    """Engine.maf_chunk over the blocks' chunk records in windows of at most `window_records` records (a window may end
    inside a block: the rows' carries cross it)"""
    text, rows = bytearray(), []
    for blk in blocks:
        for (name, start, _size, strand, src, seq) in blk:
            name_off = len(text)
            text += name
            seq_off = len(text)
            text += seq + b"\n"
            rows.append((seq_off, len(seq), name_off, start, src, len(name), 1 if strand == b"-" else 0))
    text += b"\0" * 16
    d_text = eng.upload(np.frombuffer(bytes(text), dtype=np.uint8))
    d_rows = eng.upload(np.array(rows, dtype=MAF_CHUNK_ROW_DTYPE))
    carry = eng.upload(np.zeros(max(len(rows), 1), dtype=np.uint64))
    recs, row0 = [], 0
    for blk in blocks:
        nk = len(ref.chunk_bounds(len(blk[0][5]), L))
        recs += [(row0, len(blk), k) for k in range(nk)]
        row0 += len(blk)
    out = []
    for a in range(0, len(recs), window_records):
        win = []
        for (r0, nr, k) in recs[a:a + window_records]:
            if win and win[-1][0] == r0:
                win[-1][2] = k + 1
            else:
                win.append([r0, k, k + 1, nr, 0])
        out.append(eng.maf_chunk(d_text, d_rows, np.array([tuple(w) for w in win], dtype=MAF_CHUNK_BLOCK_DTYPE), L, carry))
    return b"".join(out)


ABI_SHAPES = [  # (seed, blocks, most columns, L, window records)
    (1, 20, 300, 7, 5), (2, 12, 700, 32, 3), (3, 12, 700, 31, 1000), (4, 10, 2100, 33, 4), (5, 6, 4200, 2048, 2),
    (6, 6, 4200, 2047, 1), (7, 8, 200, 1, 150), (8, 10, 3000, 64, 7), (9, 5, 2049, 2049, 1), (10, 30, 90, 1000, 4),
]


def check_abi_shapes(eng, shapes=ABI_SHAPES):
    for seed, nb, cols, L, win in shapes:
        blocks = random_blocks(seed, nb, cols, longer=True)
        text, panic = ref.chunk_text(blocks, L)
        assert panic is None, seed
        got = abi_chunk(eng, blocks, L, win)
        assert got == text, (seed, L, win)


def check_abi_long_rows(eng, cols=40000, L=9000):
    """rows beyond maf_long_cols (32 768) and a window boundary inside the block"""
    blocks = random_blocks(77, 2, 10, longer=False)
    rng = random.Random(5)
    blocks.insert(1, [(b"big%d" % r, 10 ** r, 0, b"+", 10 ** 9, _row_text(rng, cols)) for r in range(3)])
    text, panic = ref.chunk_text(blocks, L)
    assert panic is None
    assert abi_chunk(eng, blocks, L, 2) == text
    assert abi_chunk(eng, blocks, L, 1000) == text


TILE = 8192                                                              # bytes of text per fill block (WGA_MAF_TILE)
U64 = (1 << 64) - 1


def check_one_window(eng, blocks, L, window_records=10 ** 9):
    text, panic = ref.chunk_text(blocks, L)
    assert panic is None
    got = abi_chunk(eng, blocks, L, window_records)
    assert got == text, (L, window_records, len(got), len(text))
    return text


def lead(nbytes, name=b"L"):
    """a one-row block whose only record (L >= its columns) is exactly nbytes long"""
    for n in range(max(nbytes - 40, 0), nbytes):
        blk = [(name, 0, 0, b"+", 0, b"A" * n)]
        if len(ref.chunk_text([blk], 10 ** 6)[0]) == nbytes:
            return blk
    raise AssertionError(nbytes)


def short(i, rows=2):
    return [(b"s%d.%d" % (i, r), 10 * i + r, 0, b"-" if (i + r) % 3 == 0 else b"+", 1000 + i, b"AC-GT-A") for r in range(rows)]


def check_abi_record_ends_at_tile_edge(eng):
    """the lead block's record ends with byte 8190 .. 8193 of the window's text (8191, 8192 and 8193 counted from 0 or from
    1); two short two-row blocks follow"""
    for nbytes in (TILE - 1, TILE, TILE + 1, TILE + 2):
        blocks = [lead(nbytes), short(1), short(2)]
        text = check_one_window(eng, blocks, 10 ** 6)
        assert text[nbytes - 2:nbytes + 12] == b"\n\na score=255\n"
        check_one_window(eng, blocks, 10 ** 6, window_records=2)          # ... and with the window's end behind the edge


def check_abi_fields_straddle_tile_edge(eng):
    """the second block's first line starts 120 .. 0 bytes in front of byte 8192: the edge falls into `a score`, the name, each
    number (start and srcSize hold 20 digits), the strand and the slice in turn"""
    two = [(b"chrStraddle", U64 - 1, 0, b"-", U64 - 2, b"ACGT" * 9), (b"chrStraddlf", U64 - 37, 0, b"-", U64, b"-" * 36)]
    for gap in range(0, 121):
        blocks = [lead(TILE - gap), two, short(3)]
        text = check_one_window(eng, blocks, 10 ** 6)
        assert text[TILE - gap:TILE - gap + 12] == b"a score=255\n"


def check_abi_many_lines_per_tile(eng, n=700):
    """L = 1 over n one-column two-row blocks with empty names: 13-byte lines, the most a tile meets.  A one-column block is
    one record, so one three-column block stands in the middle and the windows are cut after its first record: the boundary
    lies inside it and its rows' carries cross it"""
    one = [[(b"", b, 0, b"+", 0, b"A"), (b"", 0, 0, b"-", 9, b"-")] for b in range(n)]
    mid = [(b"", 5, 0, b"+", 0, b"A-C"), (b"", 6, 0, b"+", 0, b"GT-")]
    blocks = one[:n // 2] + [mid] + one[n // 2:]
    check_one_window(eng, blocks, 1)
    check_one_window(eng, blocks, 1, window_records=n // 2 + 1)


# ---- command line ----------------------------------------------------------------------------------------------------------
def fixture_expected():
    return open(os.path.join(GOLDEN, "test_chunk_l300.maf"), "rb").read()


def check_fixture(cli):
    rc, out, err = run(cli, "chunk", os.path.join(GOLDEN, "test.maf"), "-l", "300")
    assert rc == 0, err
    assert out == fixture_expected()
    rc, out2, err = run(cli, "ch", "--length=300", os.path.join(GOLDEN, "test.maf"))
    assert rc == 0, err
    assert out2 == out
    rc, out3, err = run(cli, "ch", "--length", "300", stdin=open(os.path.join(GOLDEN, "test.maf"), "rb").read())
    assert rc == 0, err
    assert out3 == out


LENGTHS = [1, 2, 31, 32, 33, 63, 64, 65, 1000, 2 ** 63]


def check_random_files(cli, tmp_path, seeds=(11, 12), n_blocks=14, max_cols=260):
    for seed in seeds:
        blocks = random_blocks(seed, n_blocks, max_cols, max_rows=40 if seed % 2 else 5)
        path = str(tmp_path / ("r%d.maf" % seed))
        open(path, "wb").write(maf_text(blocks, seed=seed))
        bl = len(blocks[0][0][5])
        for L in LENGTHS + [max(bl - 1, 1), bl, bl + 1]:
            exp, panic = expected(blocks, L)
            rc, out, err = run(cli, "chunk", path, "-l", str(L))
            if panic is None:
                assert rc == 0, (seed, L, err)
                assert out == exp, (seed, L)
            else:
                assert rc == 1 and "panic" in err, (seed, L, err)
                assert out == exp, (seed, L)


def good_blocks(seed, n_blocks, max_cols, max_rows=6):
    """random blocks without short rows (every record can be written)"""
    blocks = random_blocks(seed, n_blocks, max_cols, max_rows=max_rows)
    return [[r if len(r[5]) >= len(rows[0][5]) else r[:5] + (r[5] + b"A" * (len(rows[0][5]) - len(r[5])),)
             for r in rows] for rows in blocks]


def check_readers_pieces_windows(cli, tmp_path):
    """stdin, .gz output, bgzipped input, the host reader, many pieces and many windows (a record above the budget): one
    set of bytes"""
    from cli_cases import _bgzf_write
    blocks = good_blocks(21, 25, 400)
    data = maf_text(blocks, seed=3)
    path = str(tmp_path / "in.maf")
    open(path, "wb").write(data)
    bgz = str(tmp_path / "in.maf.gz")
    _bgzf_write(bgz, data, block=3000)
    for L in (1, 45, 1000):
        exp, panic = expected(blocks, L)
        assert panic is None
        outs = [run(cli, "chunk", path, "-l", str(L)),
                run(cli, "chunk", "-l", str(L), stdin=data),
                run(cli, "chunk", bgz, "-l", str(L)),
                run(cli, "chunk", path, "-l", str(L), env={"WGA_MAF_READER": "host"}),
                run(cli, "chunk", path, "-l", str(L), env={"WGA_CHUNK_BYTES": "3000"}),
                run(cli, "chunk", path, "-l", str(L), env={"WGA_MAF_CHUNK_OUT_BYTES": "700"}),
                run(cli, "chunk", path, "-l", str(L), env={"WGA_MAF_CHUNK_OUT_BYTES": "1", "WGA_CHUNK_BYTES": "999"})]
        for rc, out, err in outs:
            assert rc == 0, err
            assert out == exp, L
        gz = str(tmp_path / "o.maf.gz")
        rc, _, err = run(cli, "-r", "-o", gz, "chunk", path, "-l", str(L))
        assert rc == 0, err
        assert gzip.decompress(open(gz, "rb").read()) == exp


def check_empty_inputs(cli, tmp_path):
    for content in (b"", b"##maf version=1\n", b"##maf version=1\n\n# only comments\n"):
        path = str(tmp_path / "e.maf")
        open(path, "wb").write(content)
        rc, out, err = run(cli, "chunk", path, "-l", "10")
        assert rc == 0, err
        assert out == ref.header(10)


def check_errors(cli, tmp_path):
    src = os.path.join(GOLDEN, "test.maf")
    o = str(tmp_path / "o.maf")
    rc, out, err = run(cli, "-o", o, "chunk", src, "-l", "0")
    assert rc == 1 and "`length` should be greater than 0" in err and not os.path.exists(o)
    rc, out, err = run(cli, "chunk", src)
    assert rc != 0 and "--length" in err
    rc, out, err = run(cli, "chunk", src, "-l", "abc")
    assert rc != 0 and "--length" in err and "greater than 0" not in err
    rc, out, err = run(cli, "-o", o, "chunk", src, "-l", "300")
    assert rc == 0 and open(o, "rb").read() == fixture_expected()
    rc, out, err = run(cli, "-o", o, "chunk", src, "-l", "300")
    assert rc == 1 and open(o, "rb").read() == fixture_expected()    # the overwrite guard
    rc, out, err = run(cli, "-r", "-o", o, "chunk", src, "-l", "100")
    assert rc == 0
    missing = str(tmp_path / "missing.maf")
    o2 = str(tmp_path / "o2.maf")
    rc, out, err = run(cli, "-o", o2, "chunk", missing, "-l", "10")
    assert rc == 1 and os.path.exists(o2)


def short_row_case(tmp_path):
    blocks = good_blocks(31, 8, 300)
    rows = blocks[5]
    bl = len(rows[0][5])
    short = rows[-1][:5] + (rows[-1][5][:max(bl - 90, 1)],)
    blocks[5] = rows[:-1] + [short] if len(rows) > 1 else rows + [short]
    path = str(tmp_path / "short.maf")
    open(path, "wb").write(maf_text(blocks, seed=8))
    return path, blocks


def bad_line_case(tmp_path):
    blocks = good_blocks(32, 9, 300)
    text = maf_text(blocks[:6], seed=9) + b"a score=1\ns q 1 2 + 3 AC extra\ns r 1 2 + 3 AC\n\n" + maf_text(blocks[6:], seed=9)[26:]
    path = str(tmp_path / "bad.maf")
    open(path, "wb").write(text)
    return path, blocks[:6]


def check_stream_errors(cli, tmp_path, gpus=None):
    extra = ["--gpus", str(gpus)] if gpus else []
    path, blocks = short_row_case(tmp_path)
    for L in (7, 64, 100000):
        exp, panic = expected(blocks, L)
        assert panic is not None
        rc, out, err = run(cli, *extra, "chunk", path, "-l", str(L))
        assert rc == 1 and "panic" in err, err
        assert out == exp, L
    path, blocks = bad_line_case(tmp_path)
    exp, panic = expected(blocks, 50)
    rc, out, err = run(cli, *extra, "chunk", path, "-l", "50")
    assert rc == 1 and "Surplus" in err, err
    assert out == exp


def check_gpus(cli, tmp_path, counts=(2, 3)):
    blocks = good_blocks(41, 23, 500)
    path = str(tmp_path / "g.maf")
    open(path, "wb").write(maf_text(blocks, seed=4))
    for L in (3, 100, 600):
        one = run(cli, "chunk", path, "-l", str(L))
        assert one[0] == 0 and one[1] == expected(blocks, L)[0]
        for g in counts:
            assert run(cli, "--gpus", str(g), "chunk", path, "-l", str(L))[:2] == one[:2], (g, L)
            assert run(cli, "--gpus", str(g), "chunk", path, "-l", str(L), env={"WGA_CHUNK_BYTES": "4000",
                                                                                   "WGA_MAF_CHUNK_OUT_BYTES": "900"})[:2] == one[:2]
    for g in counts:
        check_stream_errors(cli, tmp_path, gpus=g)
