"""`maf-index` / `maf-ext` cases: the C-ABI entry (Engine.maf_slice, K21) hit by hit and the two command lines, against the
restatement in maf_ext_ref.py.  Imported by test_emu_maf_ext.py (emulator build, CPU) and test_gpu_maf_ext.py (the product on
a GPU); each provides the `cli` and `eng` fixtures."""
import gzip
import json
import os
import random

import numpy as np

import maf_ext_ref as ref
from helpers import GOLDEN
from maf_chunk_cases import _row_text, maf_text, random_blocks, run
from wgatools_amd.engine import MAF_SLICE_HIT_DTYPE, MAF_SLICE_ROW_DTYPE


# ---- ABI level -------------------------------------------------------------------------------------------------------------
def abi_expected(blocks, hits):
    """[text of hit 0, ...] up to the first hit that panics, and that hit's index (or None)"""
    out = []
    for k, (b, ord_, lo, hi, whole) in enumerate(hits):
        rows = blocks[b]
        if whole:
            out.append(ref.record_text(rows))
            continue
        try:
            out.append(ref.record_text(ref.slice_rows(rows, rows[ord_][1] + lo, rows[ord_][1] + hi, ord_)[0]))
        except ref.Panic:
            return out, k
    return out, None


def abi_slice(eng, blocks, hits):
    """Engine.maf_slice over hits = [(block, ord, cut_lo, cut_hi, whole)]; checks the text hit by hit (the binding puts guard
    bytes around d_out and checks them)"""
    text, rows, row0 = bytearray(), [], []
    for blk in blocks:
        row0.append(len(rows))
        for (name, start, asize, strand, src, seq) in blk:
            name_off = len(text)
            text += name
            seq_off = len(text)
            text += seq + b"\n"
            rows.append((seq_off, len(seq), name_off, start, asize, src, len(name), 1 if strand == b"-" else 0))
    text += b"\0" * 16
    d_text = eng.upload(np.frombuffer(bytes(text), dtype=np.uint8))
    d_rows = eng.upload(np.array(rows, dtype=MAF_SLICE_ROW_DTYPE)) if rows else eng.empty(1, MAF_SLICE_ROW_DTYPE)
    h = np.array([(row0[b], lo, hi, len(blocks[b]), ord_, 1 if whole else 0, 0) for (b, ord_, lo, hi, whole) in hits],
                 dtype=MAF_SLICE_HIT_DTYPE)
    got, short = eng.maf_slice(d_text, d_rows, h)
    exp, exp_short = abi_expected(blocks, hits)
    assert short == exp_short
    at = 0
    for k, e in enumerate(exp):
        assert got[at:at + len(e)] == e, (k, hits[k][1:])
        at += len(e)
    assert at == len(got)


_gappy = _row_text


def boundary_cuts(n_bases):
    """bases on, one before and one after every multiple of 32 and of 2048, and the row's ends"""
    pts = {0, 1, n_bases - 1, n_bases, n_bases + 1, n_bases + 5}
    for m in list(range(32, n_bases + 33, 32)) if n_bases <= 200 else [32, 64, 2048, 4096]:
        pts |= {m - 1, m, m + 1}
    return sorted(p for p in pts if p >= 0)


def check_abi_widths(eng):
    """rows of 1 .. 4097 columns: cuts whose COLUMNS fall on, before and behind every 32- and 2048-column boundary (a gap-free
    anchor: base = column) and the same cuts on gappy rows"""
    rng = random.Random(21)
    for cols in (1, 31, 32, 33, 2047, 2048, 2049, 4097):
        plain = bytes(rng.choice(b"ACGT") for _ in range(cols))
        blocks = [[(b"anc", 7, cols, b"+", 10 ** 6, plain),
                   (b"q1", 10 ** 19 + 5, 3, b"-", 2 ** 64 - 1, _gappy(rng, cols)),
                   (b"q2.long", 0, 0, b"+", 9, _gappy(rng, cols + 9))],
                  [(b"g0", 100, 0, b"+", 5000, _gappy(rng, cols)), (b"g1", 5, 0, b"-", 5000, _gappy(rng, cols))]]
        pts = boundary_cuts(cols)
        hits = []
        for lo in pts:
            for hi in pts:
                if lo <= hi and (hi - lo < 3 or (lo + hi) % 3 == 0):
                    hits.append((0, 0, lo, hi, False))
        nb = cols - blocks[1][0][5].count(b"-")
        for lo in boundary_cuts(nb):
            for hi in (lo, lo + 1, nb, nb + 3):
                if lo <= hi:
                    hits.append((1, 0, lo, hi, False))
                    hits.append((1, 1, min(lo, 3), hi, False))      # ord 1: rows may come out short (a panic ends the text)
        hits.append((0, 0, 0, 0, True))
        abi_slice(eng, blocks, [h for h in hits if not (h[0] == 1 and h[1] == 1)])
        # the ord-1 hits one by one where they panic, together where they do not
        ok = [h for h in hits if h[0] == 1 and h[1] == 1 and abi_expected(blocks, [h])[1] is None]
        abi_slice(eng, blocks, ok[:40])


def check_abi_all_gap_rows(eng):
    """an anchor without a base: col(p) = the row's length for every p; an other row of gaps only has size 0"""
    for cols in (1, 33, 2048, 2100):
        blocks = [[(b"gaps", 5, 0, b"+", 9, b"-" * cols), (b"x", 1, 0, b"+", 9, b"A" * cols), (b"y", 1, 0, b"-", 9, b"-" * cols)]]
        hits = [(0, 0, lo, hi, False) for lo in (0, 1, 5) for hi in (lo, lo + 1, 4000)]
        hits += [(0, 1, lo, hi, False) for (lo, hi) in ((0, 1), (0, cols), (cols - 1, cols), (cols, cols + 2))]
        abi_slice(eng, blocks, hits)


def check_abi_long_gap_run(eng):
    """3 000 gap columns in the anchor across two directory entries: the select skips stretches that hold no base"""
    rng = random.Random(5)
    for lead in (0, 1500, 2047, 2048):
        anc = bytes(rng.choice(b"ACGT") for _ in range(lead)) + b"-" * 3000 + b"ACGTAC" + b"-" * 40
        blocks = [[(b"a", 0, lead + 6, b"+", 10 ** 5, anc), (b"b", 50, 0, b"-", 10 ** 5, _gappy(rng, len(anc)))]]
        n = lead + 6
        hits = [(0, 0, lo, hi, False) for lo in {0, max(lead - 1, 0), lead, lead + 1, n - 1, n} for hi in (lead, lead + 1, n - 1, n, n + 1)
                if lo <= hi]
        abi_slice(eng, blocks, hits)


def check_abi_many_hits_one_block(eng, n_hits=5000):
    """hits far outnumber blocks: 0 .. 3 bases each on one 3 000-column block"""
    rng = random.Random(9)
    blocks = [[(b"t", 1000, 0, b"+", 10 ** 6, _gappy(rng, 3000)), (b"q", 77, 0, b"-", 10 ** 6, _gappy(rng, 3000))]]
    nb = 3000 - blocks[0][0][5].count(b"-")
    hits = []
    for _ in range(n_hits):
        lo = rng.randint(0, nb)
        hits.append((0, 0, lo, lo + rng.randint(0, 3), False))
    abi_slice(eng, blocks, hits)


def check_abi_tile_edges(eng):
    """text that straddles 8 KiB tile edges with names of 1 and 200 bytes, 20-digit starts, whole and sliced hits mixed"""
    rng = random.Random(13)
    blocks = []
    for b in range(6):
        cols = rng.choice((50, 700, 2500, 9000))
        blocks.append([((b"n" if (b + r) % 2 else b"N" * 200), 10 ** 19 + rng.randint(0, 10 ** 18), rng.randint(0, cols),
                        rng.choice((b"+", b"-")), 18446744073709551615, _gappy(rng, cols)) for r in range(rng.randint(1, 4))])
    hits = []
    for _ in range(300):
        b = rng.randrange(len(blocks))
        cols = len(blocks[b][0][5])
        lo = rng.randint(0, cols)
        hits.append((b, rng.randrange(len(blocks[b])), lo, lo + rng.randint(0, cols), rng.random() < 0.2))
    hits = [h for h in hits if abi_expected(blocks, [h])[1] is None]
    assert len(hits) > 150
    abi_slice(eng, blocks, hits)


def check_abi_empty(eng):
    abi_slice(eng, [[(b"a", 0, 1, b"+", 1, b"A")]], [])


def check_abi_short_rows(eng):
    """a short row at hit 0, in the middle and at the last hit: the text ends in front of it"""
    rng = random.Random(3)
    blocks = [[(b"a", 0, 300, b"+", 999, bytes(rng.choice(b"ACGT") for _ in range(300))), (b"b", 9, 0, b"-", 999, _gappy(rng, 300))],
              [(b"a", 0, 300, b"+", 999, bytes(rng.choice(b"ACGT") for _ in range(300))), (b"s", 9, 0, b"+", 999, _gappy(rng, 100))]]
    good = [(0, 0, 5, 200, False), (1, 0, 0, 100, False), (1, 0, 0, 0, True), (0, 1, 3, 40, False)]
    bad = (1, 0, 50, 101, False)
    for at in (0, 2, 4):
        hits = good[:at] + [bad] + good[at:]
        if at == 4:
            hits = good + [bad]
        assert abi_expected(blocks, hits)[1] == min(at, 4)
        abi_slice(eng, blocks, hits)
    abi_slice(eng, blocks, [good[0], bad, good[1], bad, good[2]])


def check_abi_long_block(eng, cols=10 ** 6, cuts=64, max_width=30000):
    """one block of `cols` columns x 3 rows: the directory has hundreds of entries per row and the rank pass spreads the row
    over the grid; most cuts are at most max_width bases wide (the text stays small), four span a large part of the row"""
    rng = random.Random(17)
    unit = [_gappy(rng, 50021) for _ in range(3)]
    rows = [(b"long%d" % r, 10 ** (3 * r), 0, b"+" if r != 1 else b"-", 10 ** 12, (unit[r] * (cols // 50021 + 1))[:cols]) for r in range(3)]
    blocks = [rows]
    nb = [cols - r[5].count(b"-") for r in rows]
    hits = []
    for k in range(cuts):
        ord_ = k % 3
        lo = rng.randint(0, nb[ord_])
        w = rng.randint(0, max_width) if k % 16 else rng.randint(0, nb[ord_])
        hits.append((0, ord_, lo, min(lo + w, nb[ord_] + 2), False))
    abi_slice(eng, blocks, hits)


# ---- command line ----------------------------------------------------------------------------------------------------------
def index_of(cli, path, env=None):
    rc, _, err = run(cli, "maf-index", path, env=env)
    assert rc == 0, err
    return json.load(open(path + ".index"))


LITERAL_MAF = (b"##maf version=1\n"
               b"a score=5\n"
               b"s ref 100 8 + 1000 --ACG-TACGT--\n"
               b"s qry 50 9 - 500 TTAC--TAC-GTA\n"       # the size field says 9, the text holds 10 bases
               b"s third 7 11 + 300 A-CGTTTACG-TT\n"
               b"\n")
# worked by hand from the rules (not from the restatement): ref's bases sit in columns 2 3 4 6 7 8 9 10, third's in
# 0 2 3 4 5 6 7 8 9 11 12
LITERAL_CASES = [
    ("ref:102-105",   # inside: cut 2..5 -> columns [4, 8)
     b"a score=255\ns\tref\t102\t3\t+\t1000\tG-TA\ns\tqry\t52\t2\t-\t500\t--TA\ns\tthird\t9\t4\t+\t300\tTTTA\n\n"),
    ("ref:100-102",   # cut_lo = 0: the gap columns 0 and 1 in front of the first base are dropped -> [2, 4)
     b"a score=255\ns\tref\t100\t2\t+\t1000\tAC\ns\tqry\t50\t2\t-\t500\tAC\ns\tthird\t7\t2\t+\t300\tCG\n\n"),
    ("ref:106-200",   # the block's end: cut 6..8, col(8) = the row's length -> [9, 13), the trailing gap columns are kept
     b"a score=255\ns\tref\t106\t2\t+\t1000\tGT--\ns\tqry\t56\t3\t-\t500\t-GTA\ns\tthird\t13\t3\t+\t300\tG-TT\n\n"),
    ("ref:0-1000",    # whole: every field as it is, qry's wrong size included
     b"a score=255\ns\tref\t100\t8\t+\t1000\t--ACG-TACGT--\ns\tqry\t50\t9\t-\t500\tTTAC--TAC-GTA\n"
     b"s\tthird\t7\t11\t+\t300\tA-CGTTTACG-TT\n\n"),
    ("third:9-12",    # ord = 2: cut 2..5 of third -> [3, 6); the other rows' starts get cut_lo = 2 added
     b"a score=255\ns\tref\t102\t2\t+\t1000\tCG-\ns\tqry\t52\t1\t-\t500\tC--\ns\tthird\t9\t3\t+\t300\tGTT\n\n"),
    ("ref:103-103",   # start == end inside the block: a hit with empty slices
     b"a score=255\ns\tref\t103\t0\t+\t1000\t\ns\tqry\t53\t0\t-\t500\t\ns\tthird\t10\t0\t+\t300\t\n\n"),
]
EXT_HEADER = b"#maf version=1.6 cmd=maf_extract\n"


def check_literal(cli, tmp_path):
    path = str(tmp_path / "lit.maf")
    open(path, "wb").write(LITERAL_MAF)
    index_of(cli, path)
    for region, exp in LITERAL_CASES:
        rc, out, err = run(cli, "maf-ext", path, "-r", region)
        assert rc == 0, err
        assert out == EXT_HEADER + exp, region
        assert "WARN" not in err
    rc, out, err = run(cli, "me", path, "--regions", ",".join(["nope:1-5"] + [r for r, _ in LITERAL_CASES] + ["ref:500-600"]))
    assert rc == 0, err
    assert out == EXT_HEADER + b"".join(e for _, e in LITERAL_CASES)
    warns = [ln.split(" WARN ", 1)[1] for ln in err.splitlines() if " WARN " in ln]
    assert warns == ["Failed region: nope:1-5", "Failed region: ref:500-600"]
    # the restatement agrees with the hand-worked bytes
    idx, e = ref.build_index(LITERAL_MAF)
    text, failed, panic = ref.extract(LITERAL_MAF, idx, [ref.parse_region(r.encode()) for r, _ in LITERAL_CASES])
    assert panic is None and text == EXT_HEADER + b"".join(e for _, e in LITERAL_CASES)


def unique_names(blocks):
    return [[(b"b%d_" % b + r[0],) + r[1:] for r in rows] for b, rows in enumerate(blocks)]


def check_index_fixtures(cli, tmp_path):
    import shutil
    for name in ("test_chunk_l300.maf", "test.maf"):
        path = str(tmp_path / name)
        shutil.copy(os.path.join(GOLDEN, name), path)
        exp, e = ref.build_index(open(path, "rb").read())
        assert e is None
        assert index_of(cli, path) == exp, name


def check_index_random(cli, tmp_path):
    for seed in (51, 52, 53):
        blocks = unique_names(random_blocks(seed, 30, 200))
        data = maf_text(blocks, noise=True, seed=seed)
        path = str(tmp_path / ("i%d.maf" % seed))
        open(path, "wb").write(data)
        exp, e = ref.build_index(data)
        assert e is None
        got = [index_of(cli, path, env=env) for env in (None, {"WGA_CHUNK_BYTES": "200"}, {"WGA_CHUNK_BYTES": "4096"},
                                                         {"WGA_MAF_READER": "host"})]
        for g in got:
            assert g == exp, seed
        assert [b[0] for b in ref.blocks_with_offsets(data)] == sorted({iv["offset"] for v in exp.values() for iv in v["ivls"]})


def check_index_errors_and_output(cli, tmp_path):
    def write(name, body):
        p = str(tmp_path / name)
        open(p, "wb").write(b"##maf version=1\n" + body)
        return p
    p = write("dup.maf", b"a\ns x 0 2 + 9 AC\ns x 3 2 + 9 AC\n\n")
    rc, _, err = run(cli, "maf-index", p)
    assert rc == 1 and "Duplicate name `x` in a record not allowed, please check or use `rename`" in err
    p = write("both.maf", b"a\ns x 0 2 + 9 AC\ns y 3 2 + 9 AC\n\na\ns y 0 2 + 9 AC\ns x 3 2 + 9 AC\n\n")
    rc, _, err = run(cli, "mi", p)
    assert rc == 1 and "Same sequence cannot be both reference and query!" in err
    p = write("empty.maf", b"\n# nothing\n")
    rc, _, err = run(cli, "maf-index", p)
    assert rc == 1 and "Empty record" in err
    good = b"a\ns na\"me\\z 4 2 + 9 AC\ns y 3 2 - 9 A-C\ns c\x01t\x1fl 0 1 + 9 --A\n\n"
    p = write("good.maf", good)
    other = str(tmp_path / "other.json")
    rc, _, err = run(cli, "-o", other, "maf-index", p)
    assert rc == 0 and not os.path.exists(p + ".index"), err
    exp, _ = ref.build_index(b"##maf version=1\n" + good)
    assert json.load(open(other)) == exp and 'na"me\\z' in exp and "c\x01t\x1fl" in exp
    assert b'"c\\u0001t\\u001fl"' in open(other, "rb").read()                        # control bytes as serde_json writes them
    assert b" " not in open(other, "rb").read().replace(b'"na\\"me\\\\z"', b"")     # compact, one line
    open(p + ".index", "w").write("stale")
    rc, _, err = run(cli, "maf-index", p)                                              # overwritten without -r
    assert rc == 0 and json.load(open(p + ".index")) == exp


def check_index_refuses_compressed(cli, tmp_path):
    """the reference reads the file as it is and maf-ext preads at the offsets: a .gz cannot be indexed, and is not inflated"""
    from cli_cases import _bgzf_write
    data = maf_text(unique_names(random_blocks(61, 5, 80)), seed=1)
    for name, write in (("p.maf.gz", lambda p: open(p, "wb").write(gzip.compress(data))), ("b.maf.gz", lambda p: _bgzf_write(p, data, block=500))):
        path = str(tmp_path / name)
        write(path)
        rc, _, err = run(cli, "maf-index", path)
        assert rc == 1 and "reads the file as it is" in err, err
        assert not os.path.exists(path + ".index")


def check_index_then_call(cli, tmp_path):
    """loop closure: the index maf-index writes is the one `call` reads for its ##contig lines"""
    import shutil
    path = str(tmp_path / "t.maf")
    shutil.copy(os.path.join(GOLDEN, "test.maf"), path)
    rc, before, err = run(cli, "call", path)
    assert rc == 0 and b"##contig" not in before, err
    exp = index_of(cli, path)
    rc, out, err = run(cli, "call", path)
    assert rc == 0, err
    got = [ln for ln in out.split(b"\n") if ln.startswith(b"##contig")]
    want = {b"##contig=<ID=%s,length=%d>" % (k.encode(), n) for k, n in ref.ref_contigs(exp)}
    assert want and set(got) == want and len(got) == len(want)


def battery_file(seed):
    """blocks on one reference in touching intervals, queries q1 / q2 (q2 not in every block), every row as long as the block"""
    rng = random.Random(seed)
    blocks, at = [], rng.randint(0, 50)
    for b in range(rng.randint(3, 9)):
        cols = rng.choice((1, 31, 32, 33, 64, 100, 257, 2049, 2300)) if rng.random() < 0.5 else rng.randint(1, 400)
        rows = []
        for r, name in enumerate((b"chrA", b"q1", b"q2")):
            if r == 2 and rng.random() < 0.4:
                continue
            seq = _row_text(rng, cols)
            n = cols - seq.count(b"-")
            start = at if r == 0 else rng.randint(0, 5000)
            rows.append((name, start, n + (1 if rng.random() < 0.1 else 0), b"+" if r == 0 or rng.random() < 0.5 else b"-", 10 ** 6, seq))
            if r == 0:
                at += n + (0 if rng.random() < 0.6 else rng.randint(1, 30))
        blocks.append(rows)
    return blocks


def battery_regions(rng, blocks, n):
    ivs = [(r[0], r[1], r[1] + r[2]) for rows in blocks for r in rows]
    out = []
    while len(out) < n:
        name, s, e = rng.choice(ivs)
        k = rng.random()
        if k < 0.12:
            out.append((name, max(s - rng.randint(0, 3), 0), e + rng.randint(0, 3)))          # whole
        elif k < 0.45 and e > s:
            a = rng.randint(s, e - 1)
            out.append((name, a, rng.randint(a, e)))                                          # partial (zero-length too)
        elif k < 0.6:
            out.append((b"chrA", max(s - rng.randint(0, 200), 0), e + rng.randint(0, 600)))  # over several blocks
        elif k < 0.7:
            out.append((name, s, s + 1) if rng.random() < 0.5 else (name, max(e - 1, s), e))  # touching the ends
        elif k < 0.78 and out:
            out.append(rng.choice(out))                                                       # duplicated
        elif k < 0.84:
            out.append((name, s + (e - s) // 2, s + (e - s) // 2))                            # zero-length
        elif k < 0.9:
            out.append((rng.choice((b"nope", b"chrB", b"q9")), s, e))                         # absent names
        elif k < 0.95:
            out.append((name, 10 ** 9, 10 ** 9 + 5))                                          # overlaps nothing
        else:
            out.append((name, e, e + rng.randint(0, 9)))                                      # just behind a block
    return out


def region_args(regions):
    return ",".join("%s:%d-%d" % (n.decode(), s, e) for n, s, e in regions)


def check_battery(cli, tmp_path, files=40, n_regions=200):
    tally = {}
    n_failed = n_total = 0
    for f in range(files):
        rng = random.Random(1000 + f)
        blocks = battery_file(2000 + f)
        data = maf_text(blocks, noise=True, seed=f)
        path = str(tmp_path / ("b%d.maf" % f))
        open(path, "wb").write(data)
        idx = index_of(cli, path)
        regions = battery_regions(rng, blocks, n_regions)
        exp, failed, panic = ref.extract(data, idx, regions, tally)
        assert panic is None
        n_failed += len(failed)
        n_total += len(regions)
        tsv = str(tmp_path / ("b%d.tsv" % f))
        open(tsv, "wb").write(b"".join(b"%s\t%d\t%d\n" % r for r in regions[n_regions // 2:]))
        rc, out, err = run(cli, "maf-ext", path, "-r", region_args(regions[:n_regions // 2]), "-f", tsv)
        assert rc == 0, err
        assert out == exp, f
        warns = [ln.split(" WARN ", 1)[1] for ln in err.splitlines() if " WARN " in ln]
        assert warns == ["Failed region: %s:%d-%d" % (n.decode(), s, e) for n, s, e in failed]
    h = tally["hits"]
    assert tally["sliced"] >= 0.25 * h and tally["whole"] >= 0.05 * h and tally["c1_at_end"] >= 0.05 * h, tally
    assert tally["ord_gt0"] >= 0.05 * h and n_failed >= 0.02 * n_total, (tally, n_failed, n_total)


def check_ext_outputs_and_windows(cli, tmp_path):
    """-o x.maf.gz, the window budget at 1 / 300 / default, the host reader, small input pieces: one set of bytes"""
    blocks = battery_file(77)
    data = maf_text(blocks, noise=True, seed=5)
    path = str(tmp_path / "w.maf")
    open(path, "wb").write(data)
    idx = index_of(cli, path)
    regions = battery_regions(random.Random(78), blocks, 120)
    exp, failed, panic = ref.extract(data, idx, regions)
    assert panic is None
    args = ["maf-ext", path, "-r", region_args(regions)]
    for env in (None, {"WGA_MAF_EXT_OUT_BYTES": "1"}, {"WGA_MAF_EXT_OUT_BYTES": "300"}, {"WGA_MAF_READER": "host"},
                {"WGA_CHUNK_BYTES": "500"}, {"WGA_MAF_READER": "host", "WGA_MAF_EXT_OUT_BYTES": "1"}):
        rc, out, err = run(cli, *args, env=env)
        assert rc == 0, err
        assert out == exp, env
    gz = str(tmp_path / "o.maf.gz")
    rc, _, err = run(cli, "-o", gz, *args)
    assert rc == 0, err
    assert gzip.decompress(open(gz, "rb").read()) == exp
    rc, _, err = run(cli, "-o", gz, *args)
    assert rc == 1                                                       # the overwrite guard
    rc, _, err = run(cli, "--rewrite", "-o", gz, *args)
    assert rc == 0 and gzip.decompress(open(gz, "rb").read()) == exp


def check_ext_non_ascii(cli, tmp_path):
    path = str(tmp_path / "u.maf")
    data = "##maf\na score=1\ns a 5 4 + 90 AéC-GT\ns b 7 6 - 80 ACGTTAG\n\n".encode()
    open(path, "wb").write(data)
    idx = index_of(cli, path)
    # a's characters: A e-acute C - G T; bases A(0) e(1) C(2) G(3) T(4) at characters 0 1 2 4 5; bytes: A 0, e 1-2, C 3, - 4, G 5, T 6
    rc, out, err = run(cli, "maf-ext", path, "-r", "b:9-10")          # anchor b (ASCII): column 2 is the second byte of a's character
    assert rc == 1 and "char boundary" in err and out == EXT_HEADER
    rc, out, err = run(cli, "maf-ext", path, "-r", "b:10-12")         # columns [3, 5): a's bytes 3 4 = "C-"
    exp, failed, panic = ref.extract(data, idx, [(b"b", 10, 12)])
    assert panic is None and exp == EXT_HEADER + b"a score=255\ns\ta\t8\t1\t+\t90\tC-\ns\tb\t10\t2\t-\t80\tTT\n\n"
    assert rc == 0 and out == exp, err


def check_ext_short_row(cli, tmp_path):
    """a short row in hit k: the records of hits 0 .. k - 1 are written, then the panic"""
    data = (b"##maf\na\ns r 0 10 + 99 ACGTACGTAC\ns q 0 10 + 99 ACGTACGTAC\n\n"
            b"a\ns r 10 10 + 99 ACGTACGTAC\ns q 0 4 + 99 ACGT\n\na\ns r 20 5 + 99 ACGTA\n\n")
    path = str(tmp_path / "s.maf")
    open(path, "wb").write(data)
    idx = index_of(cli, path)
    regions = [(b"r", 2, 5), (b"r", 11, 13), (b"r", 12, 17), (b"r", 21, 22)]
    exp, failed, panic = ref.extract(data, idx, regions)
    assert panic is not None and exp.count(b"a score") == 2
    for env in (None, {"WGA_MAF_EXT_OUT_BYTES": "1"}):
        rc, out, err = run(cli, "maf-ext", path, "-r", region_args(regions), env=env)
        assert rc == 1 and "panic" in err, err
        assert out == exp


def check_ext_errors(cli, tmp_path):
    path = str(tmp_path / "e.maf")
    open(path, "wb").write(LITERAL_MAF)
    o = str(tmp_path / "o.maf")
    rc, _, err = run(cli, "-o", o, "maf-ext", path)
    assert rc == 1 and "regions or region_file must be specified" in err and not os.path.exists(o)
    rc, _, err = run(cli, "-o", o, "maf-ext", "-r", "ref:1-2")
    assert rc == 1 and "Stdin not allowed here" in err and os.path.exists(o)
    rc, _, err = run(cli, "maf-ext", "-", "-r", "ref:1-2")
    assert rc == 1 and "Stdin not allowed here" in err
    rc, _, err = run(cli, "maf-ext", str(tmp_path / "missing.maf"), "-r", "ref:1-2")
    assert rc == 1
    rc, _, err = run(cli, "maf-ext", path, "-r", "ref:1-2")              # no index yet
    assert rc == 1 and ".index" in err
    open(path + ".index", "w").write('{"ref":{"ivls":[],"size":5}}')     # a missing key
    rc, _, err = run(cli, "maf-ext", path, "-r", "ref:1-2")
    assert rc == 1 and "json dese error" in err
    open(path + ".index", "w").write('{"ref":')
    rc, _, err = run(cli, "maf-ext", path, "-r", "ref:1-2")
    assert rc == 1 and "json dese error" in err
    index_of(cli, path)
    for bad in ("ref", "ref:1", "ref:a-b", "re f:1-2", "ref:1-2x"):
        rc, _, err = run(cli, "maf-ext", path, "-r", bad)
        assert rc == 1 and "Parse Genome Region Error By: Region `%s` is match the format of `chr:start-end`" % bad in err, err
    rc, _, err = run(cli, "maf-ext", path, "-r", "ref:9-3")
    assert rc == 1 and "Parse Genome Region Error By: Start `9` is larger than end `3`" in err
    tsv = str(tmp_path / "r.tsv")
    open(tsv, "w").write("ref\t9\t3\n")
    rc, _, err = run(cli, "maf-ext", path, "-f", tsv)
    assert rc == 1 and "Start `9` is larger than end `3`" in err
    open(tsv, "w").write("ref\t9\n")
    rc, _, err = run(cli, "maf-ext", path, "--file", tsv)
    assert rc == 1
    open(tsv, "w").write("re f\t102\t105\n")                             # names in the file are not checked against the pattern
    rc, out, err = run(cli, "maf-ext", path, "-f", tsv)
    assert rc == 0 and out == EXT_HEADER and "Failed region: re f:102-105" in err


def check_ext_foreign_index(cli, tmp_path):
    """an index that does not belong to the file: a plain error exit, no wrapped subtraction, no read behind the end"""
    path = str(tmp_path / "f.maf")
    open(path, "wb").write(LITERAL_MAF)
    off = ref.header_end(LITERAL_MAF)
    one = '{"ref":{"ivls":[{"start":%d,"end":%d,"strand":"+","offset":%d}],"size":1000,"isref":true}}'
    open(path + ".index", "w").write(one % (90, 108, off))          # the row starts at 100: r_start = 95 lies in front of it
    rc, out, err = run(cli, "maf-ext", path, "-r", "ref:95-104")
    assert rc == 1 and "the index does not belong to this file" in err and out == EXT_HEADER, err
    open(path + ".index", "w").write(one % (100, 108, len(LITERAL_MAF) + 1000))
    rc, out, err = run(cli, "maf-ext", path, "-r", "ref:102-104")
    assert rc == 1 and "the index does not belong to this file" in err and out == EXT_HEADER, err
    open(path + ".index", "w").write(one % (100, 108, len(LITERAL_MAF)))     # at the end of the file: no record there
    rc, out, err = run(cli, "maf-ext", path, "-r", "ref:102-104")
    assert rc == 1 and "Empty record" in err, err
    open(path + ".index", "w").write(one % (100, 123456789012345678901234567890, off))   # beyond u64
    rc, out, err = run(cli, "maf-ext", path, "-r", "ref:102-104")
    assert rc == 1 and "json dese error" in err, err


def check_ext_gpus(cli, tmp_path, counts=(2, 3)):
    """--gpus N: device g takes a contiguous range of each window's hits; the bytes of one device, the panic included"""
    blocks = battery_file(91)
    data = maf_text(blocks, noise=True, seed=6)
    path = str(tmp_path / "g.maf")
    open(path, "wb").write(data)
    idx = index_of(cli, path)
    regions = battery_regions(random.Random(92), blocks, 150)
    exp, failed, panic = ref.extract(data, idx, regions)
    assert panic is None
    args = ["maf-ext", path, "-r", region_args(regions)]
    one = run(cli, *args)
    assert one[0] == 0 and one[1] == exp
    for g in counts:
        for env in (None, {"WGA_MAF_EXT_OUT_BYTES": "2000"}, {"WGA_MAF_READER": "host", "WGA_MAF_EXT_OUT_BYTES": "1"}):
            rc, out, err = run(cli, "--gpus", str(g), *args, env=env)
            assert rc == 0, err
            assert out == exp, (g, env)
    spath = str(tmp_path / "gs.maf")
    sdata = (b"##maf\n" + b"".join(b"a\ns r %d 10 + 999 ACGTACGTAC\ns q 0 %d + 99 %s\n\n" % (10 * k, 4 if k == 5 else 10,
                                                                                             b"ACGT" if k == 5 else b"ACGTACGTAC")
                                   for k in range(8)))
    open(spath, "wb").write(sdata)
    sidx = index_of(cli, spath)
    sregions = [(b"r", 10 * k + 2, 10 * k + 7) for k in range(8)]
    sexp, _, spanic = ref.extract(sdata, sidx, sregions)
    assert spanic is not None and sexp.count(b"a score") == 5
    for g in (1,) + tuple(counts):
        rc, out, err = run(cli, "--gpus", str(g), "maf-ext", spath, "-r", region_args(sregions))
        assert rc == 1 and "panic" in err, err
        assert out == sexp, g


def check_ext_hand_written_index(cli, tmp_path):
    """reordered keys, white space, an extra key, an offset that is not a sort key"""
    path = str(tmp_path / "h.maf")
    open(path, "wb").write(LITERAL_MAF)
    off = ref.header_end(LITERAL_MAF)
    open(path + ".index", "w").write(
        '{ "ref" : {"isref": true, "extra": [1, {"a": "b"}], "size": 1000,\n  "ivls": [ {"offset": %d, "strand": "+", "end": 108, '
        '"note": null, "start": 100} ] } }\n' % off)
    rc, out, err = run(cli, "maf-ext", path, "-r", "ref:102-105,third:9-12")
    assert rc == 0, err
    assert out == EXT_HEADER + LITERAL_CASES[0][1] and "Failed region: third:9-12" in err
