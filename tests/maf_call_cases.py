"""K19 (`wga_maf_call_vcf`: chunk cuts, `after_m` rules and VCF rows of `call` on MAF) at kernel level, through the C-ABI only,
against the oracle.  Imported by test_emu_maf_call.py (emulator build, CPU) and test_gpu_maf_call.py (the product on a GPU).

The expectation is never a restatement of the rules: a clean block's text is orc.call_var_maf_record; a block with bad bases
ends in front of its first bad chunk, the chunks coming from orc.find_safe_chunk_boundary + orc.call_within_var with the
chunk's coordinates counted from the rows (expect_block; pinned against call_var_maf_record on every block it is used on).
The text buffer is [guard | text | guard]: the fill pass must leave both guards as they were."""
import functools

import numpy as np

import oracle_py as orc
from wgatools_amd.engine import MAF_VCF_REC_DTYPE, VCF_ERR_DTYPE

NONE = 0xFFFFFFFFFFFFFFFF
GUARD_BYTE = 0xA5                     # no VCF row holds it: rows are 7-bit text
GOOD = frozenset(b"ACGTNacgtn-")
IUPAC = b"RYKMSWBDHVrykmU*"
BIG = 10 ** 6                         # the command line's default chunk size


# ---- blocks ----------------------------------------------------------------------------------------------------------------
def block(t, q, t_name="chrT", q_name="qry.1", t_start=1000, q_start=2000, q_size=10 ** 8, neg=False):
    assert len(t) == len(q)
    return dict(t=bytes(t), q=bytes(q), t_name=t_name, q_name=q_name, t_start=t_start, q_start=q_start, q_size=q_size,
                neg=neg, t_align=len(t) - bytes(t).count(b"-"), q_align=len(q) - bytes(q).count(b"-"), t_size=4 * 10 ** 9)


def from_runs(runs, seed=0, alpha=b"ACGT", **kw):
    """a block from (class, columns) pairs, class one of = X I D W (cigar_cat_ext_caller); neighbours of one class are one run
    for the kernel, so the lists below never repeat a class"""
    rng = np.random.default_rng(seed)
    t, q = bytearray(), bytearray()
    for c, ln in runs:
        a = [alpha[i] for i in rng.integers(0, len(alpha), ln)]
        if c == "=":
            t += bytes(a); q += bytes(a)
        elif c == "X":
            t += bytes(a); q += bytes(next(x for x in b"ACGT" if x != v) for v in a)
        elif c == "I":
            t += b"-" * ln; q += bytes(a)
        elif c == "D":
            t += bytes(a); q += b"-" * ln
        else:
            assert c == "W"
            t += b"-" * ln; q += b"-" * ln
    return block(t, q, **kw)


def col_of(runs, idx, off=0):
    """the column of run `idx`'s column `off` (negative: from the run's end)"""
    s = sum(ln for _, ln in runs[:idx])
    return s + (off if off >= 0 else runs[idx][1] + off)


def put(b, col, ch, rows="t"):
    """a copy of the block with byte `ch` at `col` of the target row, the query row or both"""
    t, q = bytearray(b["t"]), bytearray(b["q"])
    if rows in ("t", "both"):
        assert t[col] != 45
        t[col] = ch
    if rows in ("q", "both"):
        assert q[col] != 45
        q[col] = ch
    return dict(b, t=bytes(t), q=bytes(q))


def alt_runs(n, first=0):
    """n runs, '=' of 3 columns and X of 2 in turn (run i is '=' when i + first is even)"""
    return [("=", 3) if (i + first) % 2 == 0 else ("X", 2) for i in range(n)]


def synth_maf_blocks(seed, n_blocks, cols, p=(0.55, 0.12, 0.14, 0.14, 0.05), max_m=40, max_g=12):
    """random gapped row pairs: match/mismatch stretches, insertions, deletions, both-gap columns,
    adjacent I/D runs, lower-case and N bases, both strands.  `cols`: a number, or (lo, hi) for a length per block;
    p: the shares of = / X / I / D / W stretches, of up to max_m (=) and max_g (the others) columns"""
    rng = np.random.default_rng(seed)
    lens = np.random.default_rng(seed + 7919).integers(cols[0], cols[1] + 1, n_blocks) if isinstance(cols, tuple) else None
    blocks = []
    for k in range(n_blocks):
        nc = cols if lens is None else int(lens[k])
        t, q = [], []
        while len(t) < nc:
            kind = rng.choice(5, p=list(p))
            ln = int(rng.integers(1, max_m if kind == 0 else max_g))
            alpha = np.frombuffer(b"ACGTacgtN", dtype=np.uint8)
            a = alpha[rng.integers(0, 9, ln)]
            if kind == 0:
                t += list(a); q += list(a)
            elif kind == 1:
                b = alpha[rng.integers(0, 9, ln)]
                t += list(a); q += list(b)
            elif kind == 2:
                t += [45] * ln; q += list(a)
            elif kind == 3:
                t += list(a); q += [45] * ln
            else:
                t += [45] * ln; q += [45] * ln
        t, q = bytes(t[:nc]), bytes(q[:nc])
        t_al, q_al = nc - t.count(b"-"), nc - q.count(b"-")
        blocks.append(dict(t_name="chrT%d" % (k % 3), t_start=int(rng.integers(0, 10000)), t_align=t_al, t_size=50000,
                           q_name="qry.%d" % (k % 2), q_start=int(rng.integers(0, 10000)), q_align=q_al,
                           q_size=40000, neg=bool(rng.integers(0, 2)), t=t, q=q))
    return blocks


def sprinkle(blocks, seed, share, most=2):
    """IUPAC bytes over 1 .. `most` non-gap characters of about `share` of the blocks, more of them towards the block's end (the
    larger of two draws: the first bad base of a block should often lie many runs into it)"""
    rng = np.random.default_rng(seed)
    out = []
    for b in blocks:
        if len(b["t"]) and rng.random() < share:
            for _ in range(int(rng.integers(1, most + 1))):
                col, row = int(max(rng.integers(0, len(b["t"]), 2))), "tq"[int(rng.integers(0, 2))]
                if b[row][col] != 45:
                    b = put(b, col, IUPAC[int(rng.integers(0, len(IUPAC)))], row)
        out.append(b)
    return out


# ---- the expectation -------------------------------------------------------------------------------------------------------
def run_list(b):
    """(first column, class) of the block's runs, classes as K4 numbers them (0 = 1 I 2 D 3 X 4 W)"""
    ta, qa = np.frombuffer(b["t"], dtype=np.uint8), np.frombuffer(b["q"], dtype=np.uint8)
    if not len(ta):
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    tg, qg = ta == 45, qa == 45
    cls = np.where(tg & qg, 4, np.where(tg, 1, np.where(qg, 2, np.where(ta == qa, 0, 3))))
    starts = np.flatnonzero(np.concatenate([[True], cls[1:] != cls[:-1]]))
    return starts, cls[starts]


def chunks_of(b, snp, inv, svlen, chunk):
    """[(first column, end column, the chunk's rows as the oracle writes them)]: cuts from find_safe_chunk_boundary, the
    chunk record's coordinates (create_chunk_record, caller.rs:221-265; the '-' strand's accessors maf.rs:433-450) counted
    from the rows, the rows from call_within_var"""
    t, q = b["t"], b["q"]
    total = len(t)
    tpre = np.concatenate([[0], np.cumsum(np.frombuffer(t, dtype=np.uint8) != 45)])
    qpre = np.concatenate([[0], np.cumsum(np.frombuffer(q, dtype=np.uint8) != 45)])
    out, cs = [], 0
    while cs < total:
        ce = int(orc.find_safe_chunk_boundary(t, q, cs, chunk, svlen))
        assert cs < ce <= total
        t_start, t_al = b["t_start"] + int(tpre[cs]), int(tpre[ce] - tpre[cs])
        qss, q_al = b["q_start"] + int(qpre[cs]), int(qpre[ce] - qpre[cs])
        q_start, q_end = (b["q_size"] - qss - q_al, b["q_size"] - qss) if b["neg"] else (qss, qss + q_al)
        out.append((cs, ce, orc.call_within_var(b["t_name"], b["q_name"], t[cs:ce], q[cs:ce], t_start, t_start + t_al,
                                                q_start, q_end, b["neg"], snp, svlen, inv)))
        cs = ce
    return out


def first_bad(text):
    """(row index, character) of the first REF / ALT character outside ACGTN in a chunk's rows, REF before ALT; None"""
    for r, ln in enumerate(text.splitlines()):
        f = ln.split("\t")
        for field in (f[3], "" if f[4] in ("<INV>", ".") else f[4]):
            for ch in field:
                if ch not in "ACGTN":
                    return r, ch
    return None


def expect_block(b, snp, inv, svlen, chunk, pin=True):
    """dict(text, kind, ch, raw, full, chunks, bad_chunk, bad_row): the text the kernel owes (the chunks in front of the first
    bad one), the error, `raw` = the block's one bad byte if it has exactly one, `full` = the bytes of all chunks"""
    ch = chunks_of(b, snp, inv, svlen, chunk)
    whole = "".join(c[2] for c in ch)
    if pin:   # the helper against the reference's own chunk loop (it knows nothing of bad bases: the same rows either way)
        assert whole == orc.call_var_maf_record(b["t_name"], b["q_name"], b["t"], b["q"], b["t_start"], b["q_start"],
                                                b["q_align"], b["q_size"], b["neg"], snp, inv, svlen, chunk), "chunk helper"
    e = dict(kind=0, ch=None, full=len(whole), chunks=ch, bad_chunk=None, bad_row=None)
    good = []
    for k, c in enumerate(ch):
        fb = first_bad(c[2])
        if fb is not None:
            e.update(kind=2, ch=fb[1], bad_chunk=k, bad_row=fb[0])
            break
        good.append(c[2])
    e["text"] = "".join(good).encode()
    odd = [x for x in b["t"] + b["q"] if x not in GOOD]
    e["raw"] = odd[0] if len(odd) == 1 else None
    return e


def steps_of(b, e):
    """from the run list: (most 64-run steps a chunk of the block takes, the step of its chunk the first bad row's run lies in
    or None).  A row's run: the X run that holds its target base, or the next run that is not both-gap behind the run of the
    base in front of an INS / DEL; the <INV> row belongs to the chunk's first step."""
    starts, cls = run_list(b)
    if not len(starts):
        return 0, None
    ridx = lambda col: int(np.searchsorted(starts, col, side="right")) - 1
    most = max((ridx(ce - 1) - ridx(cs)) // 64 + 1 for cs, ce, _ in e["chunks"])
    if e["bad_chunk"] is None:
        return most, None
    cs, ce, text = e["chunks"][e["bad_chunk"]]
    f = text.splitlines()[e["bad_row"]].split("\t")
    if f[4] == "<INV>":
        return most, 0
    tpos = np.flatnonzero(np.frombuffer(b["t"], dtype=np.uint8) != 45)
    r = ridx(int(tpos[int(f[1]) - 1 - b["t_start"]]))
    if "SVTYPE" in f[7]:
        r += 1
        while cls[r] == 4:
            r += 1
    return most, (r - ridx(cs)) // 64


# ---- the driver ------------------------------------------------------------------------------------------------------------
def run_k19(eng, blocks, snp, inv, svlen, chunk, guard):
    """the C-ABI calls of `call` on MAF: rows up, K4 count + fill, K19 count, scan, K19 fill into [guard | text | guard].
    -> (nbytes, err, out_off, the whole buffer)"""
    n = len(blocks)
    buf, t_off, q_off, cols = bytearray(b"@"), [], [], []
    for b in blocks:                                   # filler bytes between the rows: offsets are no multiples of 16
        t_off.append(len(buf))
        buf += b["t"] + b"@@@"
        q_off.append(len(buf))
        buf += b["q"] + b"@"
        cols.append(len(b["t"]))
    buf += b"@" * 16
    names, recs = bytearray(b"#"), np.zeros(n, dtype=MAF_VCF_REC_DTYPE)
    for i, b in enumerate(blocks):
        tn, qn = b["t_name"].encode(), b["q_name"].encode()
        recs[i] = (len(names), len(names) + len(tn), len(tn), len(qn), b["t_start"], b["q_start"], b["q_size"], int(b["neg"]), 0)
        names += tn + qn
    names += b"\0"
    rows = eng.upload(np.frombuffer(bytes(buf), dtype=np.uint8))
    d_t, d_q = eng.upload(np.array(t_off, dtype=np.uint64)), eng.upload(np.array(q_off, dtype=np.uint64))
    d_c = eng.upload(np.array(cols, dtype=np.uint64))
    run_cnt = eng.maf_call_runs(n, rows, d_t, d_q, d_c)
    run_off = eng.exclusive_scan_u64(n, run_cnt)
    runs = eng.empty(3 * int(run_off.numpy()[-1]) + 3, np.uint64).fill(0)
    eng.maf_call_runs(n, rows, d_t, d_q, d_c, run_cnt=run_cnt, runs=runs, run_off=run_off)
    d_recs, d_names = eng.upload(recs), eng.upload(np.frombuffer(bytes(names), dtype=np.uint8))
    args = (n, rows, d_t, d_q, d_c, runs, run_off, d_recs, d_names, snp, inv, svlen, chunk)
    nbytes = eng.empty(n, np.uint64).fill(0xFF)
    err = eng.empty(n, VCF_ERR_DTYPE).fill(0x5A)
    eng.maf_call_vcf(*args, nbytes=nbytes, err=err)
    off = eng.exclusive_scan_u64(n, nbytes).numpy()
    n_text = int(off[-1])
    assert n_text < (1 << 40), "count pass: %r" % (nbytes.numpy()[:8],)
    out_off = off + np.uint64(guard)
    text = eng.empty(guard + n_text + guard, np.uint8).fill(GUARD_BYTE)
    eng.maf_call_vcf(*args, out=text, out_off=eng.upload(out_off))
    eng.sync()
    return nbytes.numpy(), err.numpy(), out_off, text.numpy()


def check_maf_call_vcf(eng, blocks, snp, inv, svlen, chunk, pin=True, tag=None, expect=None):
    """every block of the call against expect_block: nbytes, err.kind, err.ch, err.item (only `!= ~0` is promised for a bad
    block) and its bytes; both guards as they were.  The guards are as long as the text of ALL chunks of all blocks as the
    oracle writes it, bad characters included (a base is one byte whatever it is, so this is the length with every bad base
    replaced by a valid one of the same class): the most a fill pass that ignores the count pass's verdict can write.
    -> the expectations (for the cases' own statistics)"""
    exp = expect if expect is not None else [expect_block(b, snp, inv, svlen, chunk, pin) for b in blocks]
    guard = sum(e["full"] for e in exp) + 67
    nbytes, err, out_off, buf = run_k19(eng, blocks, snp, inv, svlen, chunk, guard)
    where = (tag, snp, inv, svlen, chunk)
    for i, e in enumerate(exp):
        assert int(nbytes[i]) == len(e["text"]), (where, i, "nbytes", int(nbytes[i]), len(e["text"]))
        assert int(err[i]["kind"]) == e["kind"], (where, i, "kind", err[i], e["ch"])
        if e["kind"]:
            got = int(err[i]["ch"])
            if e["raw"] is not None:
                assert chr(e["raw"]).upper() == e["ch"], (where, i, "the case's one bad byte is not the oracle's")
                assert got == e["raw"], (where, i, "ch", got, e["raw"])
            else:
                assert 0 < got < 128 and chr(got).upper() == e["ch"], (where, i, "ch", got, e["ch"])
            assert int(err[i]["item"]) != NONE, (where, i, "item")
        else:
            assert int(err[i]["item"]) == NONE and int(err[i]["ch"]) == 0, (where, i, err[i])
    a, z = guard, int(out_off[-1])
    assert z + guard == len(buf)
    front = np.flatnonzero(buf[:a] != GUARD_BYTE)
    back = np.flatnonzero(buf[z:] != GUARD_BYTE)
    assert not len(front), (where, "front guard", len(front), "bytes changed, the last at", int(front[-1]) - a)
    assert not len(back), (where, "back guard", len(back), "bytes changed, up to", int(back[-1]) + 1, "behind the text")
    for i, e in enumerate(exp):
        got = buf[int(out_off[i]):int(out_off[i + 1])].tobytes()
        if got != e["text"]:
            d = next((k for k in range(len(got)) if got[k] != e["text"][k]), len(got))
            assert False, (where, i, "text differs at byte", d, got[max(0, d - 60):d + 60], e["text"][max(0, d - 60):d + 60])
    return exp


# ---- parameter sets --------------------------------------------------------------------------------------------------------
HUGE = 10 ** 9     # an `svlen` larger than every gap
SVLENS = (0, 1, 2, 5, 50, HUGE)
CHUNKS = (1, 2, 7, 63, 64, 65, 300, BIG)


def params(svlens=SVLENS, chunks=CHUNKS, flags=((True, True), (False, True), (True, False), (False, False))):
    """every chunk size once and every svlen at least twice (the second time at a chunk of 63 columns and more), the flags in
    turn"""
    out, k = [], 0
    for c in chunks:
        out.append(flags[k % len(flags)] + (svlens[k % len(svlens)], c))
        k += 1
    wide = [c for c in chunks if c >= 63]
    for s in svlens:
        out.append(flags[k % len(flags)] + (s, wide[(3 * k + 1) % len(wide)]))
        k += 1
    return out


PARAMS = params()


def check_group(eng, blocks, ps, tag, thin=False):
    """the group's blocks in one call.  thin (the emulator suite, which takes milliseconds a chunk): below 63 columns a chunk
    only the blocks marked for it (`small`: the least chunk size a block is run at).  A chunk of 1, 2 or 7 columns holds a
    few runs and grows only by a gap segment, so no chunk of the hand-built blocks reaches a second 64-run step there and the
    step and carry edges do not exist at these sizes; what they exercise is cuts and chunk starts.  Dropped at 1 and 2: the
    blocks of 64 and more alternating runs, the lane-0 tails at other borders than run 64, the two 17 000-column text blocks and the three blocks of one sized step (below 63);
    at 7 the tails stay at runs 64 and 128, the run-count blocks up to 129.  cut_blocks and degenerate_blocks run whole."""
    chunk = ps[3]
    sub = [b for b in blocks if not thin or chunk >= 63 or b.get("small", 63) <= chunk]
    assert sub
    return check_maf_call_vcf(eng, sub, *ps, tag=tag)


# ---- 1. step and carry edges -----------------------------------------------------------------------------------------------
def edge_blocks():
    """hand-built run lists: a given number of runs a block, and indel rows whose run becomes lane 0 (1, 2) of a later step"""
    out = []
    for n in (1, 2, 63, 64, 65, 127, 128, 129, 1000):
        out.append(dict(from_runs(alt_runs(n), seed=n, neg=n % 2 == 1), small=1 if n <= 63 else 7 if n <= 129 else 63))
    tails = [[("I", 5)], [("D", 5)], [("W", 1), ("I", 5)], [("W", 3), ("D", 5)], [("I", 5), ("D", 5)], [("D", 6), ("I", 5)],
             [("D", 3), ("I", 6), ("D", 7), ("I", 1), ("D", 8)], [("I", 6), ("W", 2), ("D", 6)], [("W", 2)]]
    k = 0
    for at in (62, 63, 64, 65, 126, 127, 128, 129, 191, 192):      # the tail's first run has this index
        for tail in tails:
            k += 1
            if k % 3 and at not in (63, 64, 127, 128):
                continue
            # run at - 1 is '=' (k even) or X (k odd): the base in front of the tail
            runs = alt_runs(at, first=(at - 1 + k) % 2) + tail + alt_runs(8, first=k % 2) + [("D", 9), ("=", 2)]
            out.append(dict(from_runs(runs, seed=100 + k, neg=k % 4 == 0, t_name="c%d" % at, q_name="q%d" % k),
                            small=1 if at == 64 else 7 if at == 128 else 63))
    # a gap run at the very start of a block (no row, after_m false), I-D-I series
    for k, head in enumerate([[("I", 5)], [("D", 4)], [("W", 2), ("I", 3)], [("D", 3), ("W", 1), ("I", 6)], [("W", 4)],
                              [("I", 4), ("D", 4), ("I", 4), ("D", 4)]]):
        out.append(dict(from_runs(head + alt_runs(70, first=k % 2) + [("I", 3), ("D", 3), ("I", 3), ("=", 1)], seed=300 + k,
                                  neg=k % 2 == 0), small=1))
    return out


# ---- 2. chunk cuts ---------------------------------------------------------------------------------------------------------
def cut_blocks():
    """proposed ends inside '=' and X runs and gap segments shorter than, as long as and longer than the cutoffs (a segment
    of 5 and of 50 columns among them), mixed I / D / W segments, a segment of 260 runs, a segment up to the block's end"""
    a = [("=", 50), ("X", 20), ("=", 30), ("I", 3), ("D", 2), ("W", 1), ("I", 4), ("=", 40), ("D", 50), ("=", 10), ("I", 5),
         ("X", 70), ("D", 1), ("=", 64), ("I", 2), ("=", 63), ("W", 5), ("=", 60), ("D", 49), ("W", 1), ("=", 12), ("I", 200)]
    long_seg = [("=", 30)] + [(("I", "D", "W", "D", "I", "W")[i % 6], 1 + i % 3) for i in range(260)] + [("=", 30), ("X", 5)]
    tail_seg = [("X", 10), ("=", 40)] + [(("D", "I")[i % 2], 2) for i in range(150)]
    out = [from_runs(a, seed=1), from_runs(a, seed=2, neg=True, q_size=5000, q_start=100),
           from_runs(long_seg, seed=3, neg=True), from_runs(long_seg[::-1], seed=4),
           from_runs(tail_seg, seed=5), from_runs(tail_seg, seed=6, neg=True)]
    return out


# ---- 3. degenerate blocks --------------------------------------------------------------------------------------------------
def degenerate_blocks():
    one = [from_runs([(c, 1)], seed=k, neg=k % 2 == 1) for k, c in enumerate("=XIDW")]
    whole = [from_runs([(c, n)], seed=10 + k, neg=neg) for k, (c, n, neg) in enumerate(
        [("=", 300, False), ("X", 300, True), ("I", 200, True), ("D", 200, True), ("W", 100, True), ("I", 70, False),
         ("D", 70, False), ("W", 70, False)])]
    empty = block(b"", b"")
    # a '-' block whose first target base lies behind target-gap and both-gap runs, and whose chunks partly hold no target base
    late = from_runs([("I", 40), ("W", 30), ("I", 50), ("=", 5), ("X", 3), ("I", 90), ("W", 2), ("I", 70), ("D", 10), ("=", 4)],
                     seed=30, neg=True, q_size=10 ** 6)
    mix = from_runs(alt_runs(20), seed=31)
    return [mix, empty, one[0], late, empty, one[1], whole[0], one[2], whole[1], one[3], whole[2], one[4], whole[3], whole[4],
            empty, whole[5], whole[6], whole[7], dict(late, neg=False), dict(mix, neg=True), empty]


# ---- 4. text paths ---------------------------------------------------------------------------------------------------------
def sized_step_block(nbytes, t_len=11, q_len=7):
    """one block of three runs (X of 40 columns, '=', an insertion) whose single step is exactly `nbytes` bytes of text with
    -s -l 0: the insertion's length tunes it, the oracle says when it fits"""
    m = 1
    for _ in range(40):
        b = from_runs([("X", 40), ("=", 3), ("I", m)], seed=7, t_name="t" * t_len, q_name="q" * q_len, t_start=10 ** 6,
                      q_start=10 ** 6)
        have = len(orc.call_var_maf_record(b["t_name"], b["q_name"], b["t"], b["q"], b["t_start"], b["q_start"], b["q_align"],
                                           b["q_size"], False, True, False, 0, BIG))
        if have == nbytes:
            return b
        m += nbytes - have
        assert m > 0
    raise AssertionError("no insertion length gives %d bytes" % nbytes)


def text_blocks():
    mixed = b"ACGTacgtNn"
    r = [("=", 4), ("X", 300), ("=", 2), ("D", 5000), ("=", 3), ("I", 3000), ("X", 2), ("=", 1), ("D", 9000), ("X", 130)]
    small = lambda b: dict(b, small=63 if len(b["t"]) > 5000 else 1)   # the sized steps are steps at check_sized_steps' sizes only
    return [from_runs(r, seed=1, alpha=mixed, t_name="c", q_name="q"),
            from_runs(r, seed=2, alpha=mixed, t_name="T" * 200, q_name="Q" * 200, neg=True)] + [small(b) for b in _text_small(mixed)]


def _text_small(mixed):
    return [sized_step_block(8192), sized_step_block(8193), sized_step_block(8191),
            from_runs(alt_runs(150) + [("I", 9), ("=", 2), ("D", 12), ("=", 3)], seed=3, alpha=mixed, t_start=999999990,
                      q_start=3999999900, q_size=(1 << 32) + 5000),
            from_runs(alt_runs(150) + [("I", 9), ("=", 2), ("D", 12), ("=", 3)], seed=4, alpha=mixed, t_start=4 * 10 ** 9 - 40,
                      q_start=10 ** 9, q_size=(1 << 32) - 1, neg=True),
            from_runs(alt_runs(90, first=1) + [("D", 700)], seed=5, t_start=(1 << 32) - 100, q_start=5, q_size=(1 << 32) + 7,
                      neg=True)]


# ---- 5. bad bases ----------------------------------------------------------------------------------------------------------
PATTERN = [("=", 3), ("X", 2), ("=", 4), ("I", 4), ("=", 3), ("D", 4), ("=", 2), ("X", 3)]   # run i is PATTERN[i % 8]


def pattern_runs(n):
    return [PATTERN[i % 8] for i in range(n)]


def bad_base_cases():
    """(name, block, (snp, inv, svlen, chunk), where): ONE bad byte (or the same byte in both rows of an '=' column) placed by
    construction.  `where`: None = no error, else the chunk (c0 the first, c+ a later one) and the 64-run step of that chunk
    (s0, s+) the first bad row lies in; asserted against the oracle-made expectation and the run list, so a case cannot drift
    into another path"""
    R = pattern_runs(200)
    base = from_runs(R, seed=11)
    negb = from_runs(R, seed=12, neg=True)
    on = (True, True, 0)
    X100 = [("=", 5), ("X", 100), ("=", 5)]
    xb = from_runs(alt_runs(70) + X100, seed=13)
    c = lambda i, off=0: col_of(R, i, off)
    cases = [
        ("first step of the first chunk", put(base, c(1), ord("R")), on + (BIG,), "c0s0"),
        ("lane 57 of the first step", put(base, c(57), ord("y")), on + (BIG,), "c0s0"),
        ("second step of the first chunk", put(base, c(65), ord("R")), on + (BIG,), "c0s+"),
        ("a much later step of the first chunk", put(base, c(161, 1), ord("K"), "q"), on + (BIG,), "c0s+"),
        ("first step of a later chunk", put(base, c(97), ord("M")), on + (300,), "c+s0"),
        ("a later step of a later chunk", put(from_runs(pattern_runs(400), seed=14), col_of(pattern_runs(400), 361), ord("R")),
         on + (600,), "c+s+"),
        ("a later step of the second chunk", put(from_runs(pattern_runs(400), seed=15), col_of(pattern_runs(400), 289), ord("S")),
         on + (500,), "c+s+"),
        ("the last run of a block", put(base, c(199, -1), ord("W"), "q"), (True, True, HUGE, BIG), "c0s+"),
        ("the <INV> row's base", put(negb, 0, ord("U"), "both"), (False, True, 0, BIG), "c0s0"),
        ("the <INV> row's base of a later chunk", put(negb, c(94), ord("B"), "both"), (False, True, 0, 300), "c+s0"),
        ("a SNP row's REF", put(base, c(9, 1), ord("*")), on + (BIG,), "c0s0"),
        ("a SNP row's ALT", put(base, c(73), ord("d"), "q"), on + (64,), "c+s0"),
        ("the second column of a long X run", put(xb, col_of(alt_runs(70) + X100, 71, 1), ord("H")), on + (BIG,), "c0s+"),
        ("column 90 of a long X run", put(xb, col_of(alt_runs(70) + X100, 71, 90), ord("V"), "q"), on + (BIG,), "c0s+"),
        ("the base in front of an INS", put(base, c(74, -1), ord("R"), "both"), (False, False, 2, BIG), "c0s+"),
        ("the base in front of a DEL", put(base, c(132, -1), ord("r"), "both"), (False, False, 3, BIG), "c0s+"),
        ("inside a deletion's REF", put(base, c(133, 2), ord("Y")), (False, True, 0, BIG), "c0s+"),
        ("inside an insertion's ALT", put(base, c(163, 3), ord("k"), "q"), (True, False, 1, BIG), "c0s+"),
        ("inside an insertion's ALT, -c 65", put(base, c(163, 3), ord("k"), "q"), (True, False, 1, 65), "c+s0"),
        # ... and the places that raise nothing
        ("an X column without -s", put(base, c(65), ord("R")), (False, True, 0, BIG), None),
        ("a gap run of svlen columns", put(base, c(131, 1), ord("R"), "q"), (True, True, 4, BIG), None),
        ("a deletion of svlen columns", put(base, c(133, 1), ord("R")), (True, True, 4, 300), None),
        ("an '=' column no row quotes", put(base, c(130, 1), ord("R"), "both"), on + (BIG,), None),
        ("the base in front of a gap run of svlen columns", put(base, c(130, -1), ord("R"), "both"), (True, True, 4, BIG), None),
    ]
    # a gap run with after_m false: the D run behind an I run, and a gap run at the block's start
    R2 = alt_runs(66) + [("I", 5), ("D", 5), ("=", 3)] + alt_runs(70, first=1)
    cases.append(("a gap run behind a gap run", put(from_runs(R2, seed=16), col_of(R2, 67, 2), ord("R")), on + (BIG,), None))
    R3 = [("D", 6)] + alt_runs(140)
    cases.append(("a gap run at the block's start", put(from_runs(R3, seed=17), 3, ord("R")), on + (BIG,), None))
    return cases


def neighbours():
    return [from_runs(pattern_runs(50), seed=21, neg=True, t_name="n1"), from_runs(pattern_runs(90), seed=22, neg=True, q_name="n2")]


def check_bad_base_case(eng, case, arrangements=("single", "first", "middle", "last")):
    """the case's block alone, and as the first, the middle and the last of three with '-' strand neighbours"""
    name, b, (snp, inv, svlen, chunk), where = case
    e = expect_block(b, snp, inv, svlen, chunk)
    got = None if e["kind"] == 0 else ("c0" if e["bad_chunk"] == 0 else "c+") + ("s0" if steps_of(b, e)[1] == 0 else "s+")
    assert got == where, (name, "the case does not do what it was built for", got, where, e["ch"])
    n1, n2 = neighbours()
    for arr in arrangements:
        blocks = {"single": [b], "first": [b, n1, n2], "middle": [n1, b, n2], "last": [n1, n2, b]}[arr]
        check_maf_call_vcf(eng, blocks, snp, inv, svlen, chunk, tag=(name, arr))


def check_two_bad_blocks(eng):
    """each bad block reports its own error; the clean blocks between and behind them are complete"""
    cases = {c[0]: c for c in bad_base_cases()}
    n1, n2 = neighbours()
    a, b2 = cases["a much later step of the first chunk"][1], cases["second step of the first chunk"][1]
    late = cases["a later step of a later chunk"][1]
    for chunk in (BIG, 500, 64):
        exp = check_maf_call_vcf(eng, [n1, a, n2, dict(n1, neg=False), b2, late, n2], True, True, 0, chunk, tag="two bad blocks")
        assert [e["kind"] for e in exp] == [0, 2, 0, 0, 2, 2, 0]


# ---- 6. the random battery -------------------------------------------------------------------------------------------------
DENSITIES = [((0.55, 0.12, 0.14, 0.14, 0.05), 40, 12), ((0.60, 0.20, 0.09, 0.09, 0.02), 80, 6),
             ((0.30, 0.15, 0.25, 0.25, 0.05), 6, 4), ((0.45, 0.05, 0.2, 0.2, 0.1), 12, 60)]


def check_random_battery(eng, seeds, n_blocks=10, bad_share=0.5):
    """blocks of 1 .. 6 000 columns at four densities, half of them sprinkled with IUPAC bytes; four seeds of five at the
    default chunk size (a block is one chunk of many steps), the fifth at one of PARAMS' (blocks of up to 600 columns where the
    chunks are shorter than 63 columns: the emulator's time goes by the chunk).
    -> (blocks, blocks with a chunk of more than one step, bad blocks, bad blocks whose first bad row lies behind the first
    step of its chunk)"""
    tot = multi = nbad = late = 0
    for k, seed in enumerate(seeds):
        p, max_m, max_g = DENSITIES[k % len(DENSITIES)]
        snp, inv, svlen, chunk = PARAMS[(5 * k + seed) % len(PARAMS)]
        if k % 5 != 4:
            chunk, snp = BIG, k % 10 != 6
        blocks = synth_maf_blocks(seed, n_blocks, (1, 6000 if chunk >= 63 else 600), p=p, max_m=max_m, max_g=max_g)
        for b in blocks:
            b["q_size"] = 10 ** 7
        blocks = sprinkle(blocks, seed + 1, bad_share)
        exp = check_maf_call_vcf(eng, blocks, snp, inv, svlen, chunk, tag=("random", seed))
        for b, e in zip(blocks, exp):
            most, step = steps_of(b, e)
            tot += 1
            multi += most > 1
            nbad += e["kind"] == 2
            late += step is not None and step > 0
    return tot, multi, nbad, late


# ---- 7. one long block -----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=1)
def _long_block(cols, seed):
    return synth_maf_blocks(seed, 1, cols)[0]


def long_block(cols, seed=41):
    b = dict(_long_block(cols, seed))
    b["q_size"], b["neg"] = 10 ** 8, True
    return b


def check_long_block(eng, cols, chunk, pin=True):
    """a block of `cols` columns, clean and with one bad base deep inside (a SNP row's REF at 5/6 of the block).  pin: see
    expect_block; call_var_maf_record recounts the block's prefix for every chunk, so it is left out where the chunks are many"""
    clean = long_block(cols)
    col = next(k for k in range(cols * 5 // 6, cols) if 45 not in (clean["t"][k], clean["q"][k]) and clean["t"][k] != clean["q"][k])
    bad = put(clean, col, ord("R"))
    exp = check_maf_call_vcf(eng, [clean], True, True, 2, chunk, pin=pin, tag=("long", cols))
    assert exp[0]["kind"] == 0 and len(exp[0]["text"]) > cols // 10
    exp = check_maf_call_vcf(eng, [bad], True, True, 2, chunk, pin=pin, tag=("long, bad", cols))
    assert exp[0]["kind"] == 2 and exp[0]["raw"] == ord("R") and (exp[0]["bad_chunk"] > 0) == (chunk < cols // 2)
    if chunk >= 10 ** 4:
        assert steps_of(bad, exp[0])[1] > 0


# ---- shared by the two suites ----------------------------------------------------------------------------------------------
def check_block_counts(eng, n):
    blocks = (degenerate_blocks() + edge_blocks())[:n]
    for ps in ((True, True, 0, 64), (True, True, 2, BIG)):
        check_maf_call_vcf(eng, blocks, *ps, tag=("count", n))


def check_sized_steps(eng):
    """single steps of 8 191, 8 192 (the LDS stage, WGA_VCF_TB, to the byte) and 8 193 bytes (written in place)"""
    blocks = [sized_step_block(n) for n in (8191, 8192, 8193)]
    exp = check_maf_call_vcf(eng, blocks, True, False, 0, BIG, tag="sized steps")
    assert [len(e["text"]) for e in exp] == [8191, 8192, 8193] and all(len(e["chunks"]) == 1 for e in exp)
    for b in blocks:
        check_maf_call_vcf(eng, [b], True, False, 0, BIG, tag="sized step alone")


def assert_battery_shares(tot, multi, nbad, late):
    """the random battery must not go trivial: MOST blocks take more than one 64-run step in some chunk, a quarter and more of
    the blocks are bad, and a GOOD PART (a quarter and more) of the bad blocks have their first bad row behind the first step
    of its chunk: there the fill pass has clean steps in hand that belong to no reported byte, and must store none.
    Measured: the emulator suite (seeds 100 .. 114, 10 blocks each) has 150 blocks, 92 of more than one step, 54 bad, 22 of them
    behind the first step; the GPU suite (seeds 1000 .. 1059, 24 each) 1 440 blocks, 915, 536 and 246."""
    assert 2 * multi > tot, (multi, tot)
    assert 4 * nbad >= tot, (nbad, tot)
    assert 4 * late >= nbad, (late, nbad)
