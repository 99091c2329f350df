"""K31, the row frame writer of `pafpseudo` (wga_pafpseudo_frame), and the command over it: the cases the emulator and the GPU
tests share.  ABI level: every call writes into a buffer pre-filled with a sentinel, with 64 guard bytes on each side; the whole
buffer — spans, holes and guards — is compared with pseudo_frame_ref.apply."""
import os

import numpy as np

import pseudo_frame_ref as ref
from chain_split_cases import run
from pseudo_frame_ref import COPY_POOL, COPY_TEXT, FILL, HOLE
from wgatools_amd.engine import PSEUDO_FRAME_TILE, SPAN_ITEM_DTYPE

E_INVALID_ARG = -1
GUARD = 64
SENTINEL = 0xA5
T = PSEUDO_FRAME_TILE
LENS = (0, 1, 2, 15, 16, 17, 31, 32, 33, 47, 48, 49)
TEXT = np.frombuffer(b"a score=0\ns\tq1\t0\t1000\t+\t1000\t\n0123456789abcdefghijklmnopqrstuvwxyz", dtype=np.uint8)


def some_pool(n, seed=1):
    return np.random.default_rng(seed).integers(33, 127, n).astype(np.uint8)      # no byte of it is the sentinel


def tiled(spans):
    """[(len, kind, src)] -> [(dst, len, src, kind)] standing back to back, and the end"""
    items, at = [], 0
    for ln, kind, src in spans:
        items.append((at, ln, src, kind))
        at += ln
    return items, at


def as_array(items):
    a = np.zeros(len(items), dtype=SPAN_ITEM_DTYPE)
    for k, (dst, ln, src, kind) in enumerate(items):
        a[k] = (dst, ln, src, kind, 0)
    return a


def run_frame(eng, items, pool, text, out_bytes):
    """the call on a sentinel buffer with guards: (the buffer before, the buffer after, first bad item or None)"""
    before = np.full(out_bytes + 2 * GUARD, SENTINEL, dtype=np.uint8)
    buf = eng.upload(before)
    assert buf.ptr % 16 == 0
    d_pool = eng.upload(pool) if len(pool) else None                               # exactly the pool's bytes: no padding
    d_text = eng.upload(text) if len(text) else None
    bad = eng.pafpseudo_frame(as_array(items), d_pool, len(pool), d_text, len(text), buf.ptr + GUARD, out_bytes)
    eng.sync()
    return before, buf.numpy(), bad


def check(eng, items, pool=(), text=TEXT, out_bytes=None, want_bad=None):
    pool, text = np.asarray(pool, dtype=np.uint8), np.asarray(text, dtype=np.uint8)
    if out_bytes is None:
        out_bytes = items[-1][0] + items[-1][1] if items else 0
    before, got, bad = run_frame(eng, items, pool, text, out_bytes)
    want, ref_bad = ref.apply(items, pool, text, before[GUARD:GUARD + out_bytes])
    assert ref_bad == want_bad, (ref_bad, want_bad)                                # the case is what it says it is
    assert bad == want_bad, (bad, want_bad)
    assert (got[:GUARD] == SENTINEL).all() and (got[GUARD + out_bytes:] == SENTINEL).all(), "a guard byte was written"
    diff = np.nonzero(got[GUARD:GUARD + out_bytes] != want)[0]
    assert diff.size == 0, "byte %d of %d: %d, not %d (%d bytes differ)" % (diff[0], out_bytes, got[GUARD + diff[0]], want[diff[0]],
                                                                            diff.size)


def check_abi_alignment_sweep(eng):
    """COPY_POOL between two holes at every dst mod 16 x src mod 16 x length, from a pool without padding: with the slice that
    starts at the pool's byte 0 (src mod 16 == 0) and the one that ends at its last byte"""
    pool = some_pool(113)
    spans = []
    for ln in LENS:
        for d in range(16):
            for src in list(range(16)) + [len(pool) - ln]:
                spans.append(((d - sum(s[0] for s in spans)) % 16 + 16, HOLE, 0))   # the copy starts at dst mod 16 == d
                spans.append((ln, COPY_POOL, src))
    spans.append((5, HOLE, 0))
    items, _ = tiled(spans)
    assert {(dst % 16, src % 16) for dst, ln, src, kind in items if kind == COPY_POOL} >= {(d, s) for d in range(16) for s in range(16)}
    assert any(kind == COPY_POOL and src == 0 and ln == 49 for dst, ln, src, kind in items)
    assert any(kind == COPY_POOL and src + ln == len(pool) and ln == 49 for dst, ln, src, kind in items)
    check(eng, items, pool)
    items, _ = tiled([(len(pool), COPY_POOL, 0)])                                  # the whole pool, byte 0 to the last
    check(eng, items, pool)


def check_abi_fills(eng):
    """the lengths at every dst mod 16 between holes and between fills of another byte; a 16-byte group of 16 one-byte items, and
    one of all four kinds"""
    for other in (HOLE, FILL):
        spans = []
        for ln in LENS:
            for d in range(16):
                spans.append(((d - sum(s[0] for s in spans)) % 16 + 16, other, ord("-")))
                spans.append((ln, FILL, ord("N") | 0x4200))                        # only the low 8 bits of src count
        spans.append((7, other, ord("-")))
        check(eng, tiled(spans)[0])
    pool = some_pool(40, 2)
    spans = [(16, HOLE, 0)] + [(1, FILL, 65 + k) for k in range(16)] + [(16, HOLE, 0)]
    spans += [(3, FILL, ord("x")), (5, COPY_TEXT, 11), (4, COPY_POOL, 36), (4, HOLE, 0)]       # one group of four kinds
    spans += [(1, COPY_TEXT, k) for k in range(16)] + [(1, COPY_POOL, 39 - k) for k in range(16)]
    check(eng, tiled(spans)[0], pool)


def check_abi_tile_borders(eng):
    """items that end at T - 1, T and T + 1 (T = the tile size), an item over three tiles, a tile that is one hole, a tile of
    3 000 one-byte items"""
    pool = some_pool(2 * T + 100, 3)
    for kind in (FILL, COPY_POOL, HOLE):
        for end in (T - 1, T, T + 1):
            spans = [(end, kind, 7 if kind == COPY_POOL else ord("-")), (40, COPY_TEXT, 3), (T + 3 - end, FILL, ord("N"))]
            check(eng, tiled(spans)[0], pool)
    for kind in (FILL, COPY_POOL):                                                 # from the middle of tile 0 into the middle of tile 2
        spans = [(T // 2 + 5, HOLE, 0), (2 * T - 3, kind, 9 if kind == COPY_POOL else ord("-")), (30, COPY_TEXT, 0)]
        check(eng, tiled(spans)[0], pool)
    check(eng, tiled([(T - 3, FILL, ord("a")), (T + 6, HOLE, 0), (T, FILL, ord("b"))])[0])      # tile 1 is nothing but a hole
    check(eng, tiled([(T, FILL, ord("a")), (T, HOLE, 0), (T - 1, COPY_POOL, 1)])[0], pool)      # ... exactly
    rng = np.random.default_rng(4)
    spans = [(T - 100, FILL, ord("-"))]
    for k in range(3000):                                                          # over the border into the second tile
        kind = (FILL, COPY_POOL, COPY_TEXT, HOLE)[int(rng.integers(0, 4))]
        spans.append((1, kind, 33 + k % 90 if kind == FILL else int(rng.integers(0, 60))))
    spans.append((T, FILL, ord("+")))
    check(eng, tiled(spans)[0], pool)


def check_abi_empty_items_at_borders(eng):
    """runs of items without bytes in front of, on and behind a tile border: the bisection lands on the item with the byte"""
    pool = some_pool(64, 5)
    empty = [(0, FILL, ord("!")), (0, COPY_POOL, 64), (0, COPY_TEXT, 0), (0, HOLE, 0), (0, FILL, ord("?"))]
    for at in (T - 1, T, T + 1):
        spans = [(at, FILL, ord("-"))] + empty + [(1, FILL, ord("X"))] + empty + [(T + 20, FILL, ord("N"))]
        check(eng, tiled(spans)[0], pool)
    spans = empty + [(T - 1, FILL, ord("a"))] + empty + [(1, COPY_POOL, 63)] + empty + [(1, COPY_TEXT, 5)] + empty * 3 + \
            [(T - 1, HOLE, 0)] + empty + [(2, FILL, ord("b"))] + empty
    check(eng, tiled(spans)[0], pool)


def check_abi_ends(eng):
    """no item and no byte; one item; texts that do not end on a 16-byte group"""
    pool = some_pool(100, 6)
    check(eng, [], pool)
    for kind in (FILL, COPY_POOL, COPY_TEXT, HOLE):
        for ln in (0, 1, 15, 16, 17, 33):
            check(eng, tiled([(ln, kind, 2 if kind != FILL else ord("-"))])[0], pool)
    for total in (T + 1, T + 15, 2 * T - 1):
        check(eng, tiled([(total - 9, FILL, ord("-")), (4, COPY_POOL, 96), (5, COPY_TEXT, 0)])[0], pool)
        check(eng, tiled([(total - 9, COPY_POOL, 0), (9, HOLE, 0)])[0], some_pool(total - 9, 7))


def random_items(seed):
    """at most 200 items of all four kinds, lengths mixed from 0, 1..40 and 4 000..70 000, at most 1 MiB in all"""
    rng = np.random.default_rng(1000 + seed)
    pool = some_pool(80_000 + seed, seed)
    spans, total = [], 0
    for _ in range(int(rng.integers(150, 201))):
        pick = int(rng.integers(0, 10))
        ln = 0 if pick < 2 else int(rng.integers(1, 41)) if pick < 8 else int(rng.integers(4000, 70001))
        if total + ln > (1 << 20) - 200 * 40:                                      # the small ones that follow still fit
            ln = int(rng.integers(0, 41))
        kind = (FILL, COPY_POOL, COPY_TEXT, HOLE)[int(rng.integers(0, 4))]
        if kind == COPY_TEXT and ln > len(TEXT):
            kind = FILL
        src = int(rng.integers(33, 127)) if kind == FILL else int(rng.integers(0, len(pool) - ln + 1)) if kind == COPY_POOL else \
            int(rng.integers(0, len(TEXT) - ln + 1)) if kind == COPY_TEXT else int(rng.integers(0, 1 << 40))
        spans.append((ln, kind, src))
        total += ln
    items, total = tiled(spans)
    assert len(items) <= 200 and total <= (1 << 20) and {i[3] for i in items} == {FILL, COPY_POOL, COPY_TEXT, HOLE}
    return items, pool


def check_abi_random(eng, seeds=range(12)):
    for seed in seeds:
        items, pool = random_items(seed)
        check(eng, items, pool)


def check_abi_bad_items(eng):
    """a gap, an overlap, an unknown kind, a copy one byte beyond either source, a last item that ends beyond out_bytes or in
    front of it: the index, the guards, and the items in front of it are written (check compares them)"""
    pool = some_pool(50, 8)
    good = [(20, FILL, ord("-")), (9, COPY_TEXT, 1), (30, COPY_POOL, 20), (T + 5, FILL, ord("N")), (0, HOLE, 0), (17, HOLE, 0),
            (40, FILL, ord("e"))]
    items, total = tiled(good)

    def with_item(k, **kw):
        out = list(items)
        d = dict(zip(("dst", "ln", "src", "kind"), out[k]), **kw)
        out[k] = (d["dst"], d["ln"], d["src"], d["kind"])
        return out
    check(eng, items, pool, out_bytes=total)
    check(eng, with_item(3, dst=items[3][0] + 1), pool, out_bytes=total, want_bad=3)          # a gap
    check(eng, with_item(3, dst=items[3][0] - 1), pool, out_bytes=total, want_bad=3)          # an overlap
    check(eng, with_item(0, dst=1), pool, out_bytes=total, want_bad=0)                        # the first item does not start at 0
    check(eng, with_item(4, kind=4), pool, out_bytes=total, want_bad=4)
    check(eng, with_item(4, kind=0xFFFFFFFF), pool, out_bytes=total, want_bad=4)
    check(eng, with_item(2, src=21), pool, out_bytes=total, want_bad=2)                       # pool[21, 51)
    check(eng, with_item(2, src=(1 << 64) - 10), pool, out_bytes=total, want_bad=2)           # src + len wraps
    check(eng, with_item(1, src=len(TEXT) - 8), pool, out_bytes=total, want_bad=1)            # one byte beyond the text
    check(eng, with_item(6, ln=41), pool, out_bytes=total, want_bad=6)                        # the last item ends beyond out_bytes
    check(eng, with_item(6, ln=39), pool, out_bytes=total, want_bad=6)                        # ... in front of it
    check(eng, with_item(3, ln=(1 << 64) - 3), pool, out_bytes=total, want_bad=3)             # dst + len wraps
    check(eng, with_item(5, ln=1 << 63), pool, out_bytes=total, want_bad=5)
    check(eng, items, pool, out_bytes=total + 1, want_bad=6)
    check(eng, items, pool, out_bytes=total - 1, want_bad=6)                                  # only the last item leaves the text
    check(eng, items, pool, out_bytes=20, want_bad=1)


def raw(eng, n_items, items, pool, pool_bytes, text, text_bytes, out, out_bytes, first_bad):
    return eng.lib.wga_pafpseudo_frame(eng.ctx, n_items, items, pool, pool_bytes, text, text_bytes, out, out_bytes, first_bad)


def check_abi_arguments(eng):
    """null arrays and a misaligned d_out are WGA_E_INVALID_ARG, and nothing is written"""
    items, total = tiled([(20, FILL, ord("-")), (9, COPY_TEXT, 1), (30, COPY_POOL, 2)])
    d_items, d_pool, d_text = eng.upload(as_array(items)), eng.upload(some_pool(40)), eng.upload(TEXT)
    buf = eng.upload(np.full(total + 2 * GUARD, SENTINEL, dtype=np.uint8))
    fb = eng.upload(np.array([7], dtype=np.uint64))
    out = buf.ptr + GUARD
    ok = (3, d_items.ptr, d_pool.ptr, 40, d_text.ptr, len(TEXT), out, total, fb.ptr)

    def call(**kw):
        names = ("n_items", "items", "pool", "pool_bytes", "text", "text_bytes", "out", "out_bytes", "first_bad")
        return raw(eng, *[kw.get(n, v) for n, v in zip(names, ok)])
    assert call(items=None) == E_INVALID_ARG
    assert call(out=None) == E_INVALID_ARG
    assert call(first_bad=None) == E_INVALID_ARG
    assert call(pool=None) == E_INVALID_ARG
    assert call(text=None) == E_INVALID_ARG
    for shift in (1, 4, 8, 15):
        assert call(out=out + shift) == E_INVALID_ARG, shift
    assert call(n_items=0) == E_INVALID_ARG                                        # no items, but bytes
    assert call(out_bytes=1 << 47) == E_INVALID_ARG
    eng.sync()
    assert (buf.numpy() == SENTINEL).all() and int(fb.numpy()[0]) == 7
    assert call(n_items=0, items=None, out=None, out_bytes=0, pool=None, pool_bytes=0, text=None, text_bytes=0) == 0
    eng.sync()
    assert int(fb.numpy()[0]) == ref.NONE
    assert call() == 0                                                             # and the arguments as they stand are fine
    eng.sync()
    got = buf.numpy()
    want, bad = ref.apply(items, some_pool(40), TEXT, np.full(total, SENTINEL, dtype=np.uint8))
    assert bad is None and int(fb.numpy()[0]) == ref.NONE and (got[GUARD:GUARD + total] == want).all()
    assert (got[:GUARD] == SENTINEL).all() and (got[GUARD + total:] == SENTINEL).all()


def check_abi_far_offsets(eng):
    """a text of 4 GiB + 128 KiB: a few small items, one hole up to 4 GiB + 64 KiB, small items of every kind behind it; the first
    and the last 64 KiB are compared (the GPU only: the buffer is device memory that is never downloaded whole)"""
    far, edge = (1 << 32) + (64 << 10), 64 << 10
    total = far + edge
    pool = some_pool(5000, 9)
    front = [(10, COPY_TEXT, 0), (33, FILL, ord("N")), (0, HOLE, 0), (7, COPY_POOL, 4993), (1, FILL, ord("\n"))]
    back = [(3, COPY_TEXT, 10), (4000, COPY_POOL, 17), (0, COPY_POOL, 5000), (20_001, FILL, ord("-")), (35, HOLE, 0), (1, COPY_TEXT, 9),
            (16, FILL, ord("x")), (4999, COPY_POOL, 1), (1, FILL, ord("\n"))]
    n_front = sum(s[0] for s in front)
    back.insert(4, (edge - sum(s[0] for s in back), FILL, ord("y")))
    items, end = tiled(front + [(far - n_front, HOLE, 0)] + back)
    assert end == total and items[len(front) + 1][0] == far
    buf = eng.empty(total + 2 * GUARD, np.uint8).fill(SENTINEL)
    bad = eng.pafpseudo_frame(as_array(items), eng.upload(pool), len(pool), eng.upload(TEXT), len(TEXT), buf.ptr + GUARD, total)
    eng.sync()
    assert bad is None

    def part(off, n):
        h = np.empty(n, dtype=np.uint8)
        eng._check(eng.lib.wga_memcpy_d2h(eng.ctx, h.ctypes.data, buf.ptr + off, n))
        return h
    got_front, got_back = part(0, GUARD + edge), part(GUARD + far, edge + GUARD)
    want_front, _ = ref.apply(tiled(front + [(edge - n_front, HOLE, 0)])[0], pool, TEXT, np.full(edge, SENTINEL, dtype=np.uint8))
    want_back, _ = ref.apply(tiled(back)[0], pool, TEXT, np.full(edge, SENTINEL, dtype=np.uint8))
    assert (got_front[:GUARD] == SENTINEL).all() and (got_front[GUARD:] == want_front).all()
    assert (got_back[edge:] == SENTINEL).all() and (got_back[:edge] == want_back).all()
    mid = part(GUARD + (1 << 32) - 4096, 8192)                                     # the hole around 2^32 is untouched
    assert (mid == SENTINEL).all()
    buf.free()


# ---- command level -----------------------------------------------------------------------------------------------------------------
HOST_WRITER = {"WGA_PSEUDO_WRITER": "host"}
PAF_LINE = "%s\t%d\t%d\t%d\t%s\t%s\t%d\t%d\t%d\t0\t0\t60\t%s\n"


def paf_text(recs):
    return "".join(PAF_LINE % (r["qname"], r["qlen"], r["qstart"], r["qend"], r["strand"], r["tname"], r["tlen"], r["tstart"], r["tend"],
                               r["cg"]) for r in recs)


def fasta_text(contigs):
    return b"".join(b">" + name.encode() + b"\n" + b"".join(seq[k:k + 60] + b"\n" for k in range(0, len(seq), 60))
                    for name, seq in contigs.items())


def pafpseudo(cli, tmp_path, name, paf, fa=None, env=None, extra=()):
    """one run into a fresh directory under WGA_TIMING=1: (exit status, message, timing lines, {file name: bytes})"""
    import maf2paf_cases as m2p
    outdir = tmp_path / name
    args = ["pafpseudo", str(paf), "-o", str(outdir)] + (["-f", str(fa)] if fa else []) + list(extra)
    rc, _, msg, timing = m2p.timed(cli, args, env or {})
    files = {f: open(outdir / f, "rb").read() for f in sorted(os.listdir(outdir))} if os.path.isdir(outdir) else {}
    return rc, msg, timing, files


def end_to_end_input(tmp_path, base):
    """the input of cli_cases.test_pafpseudo_end_to_end, built again: 36 records over 3 targets x 3 queries with gaps, abutting,
    overlapping and contained records, in shuffled order"""
    import parity_cases as pc
    from wgatools_amd import synth
    rng = np.random.default_rng(5)
    b = synth.make_paf_batch(91, 36, 60, 60000)
    cs = synth.class_sums(b["code"], b["length"], b["op_off"])
    tspan = (cs["mx"] + cs["d"]).astype(np.int64)
    tnames, qnames = ["tA", "tB", "t10"], ["q1", "q2", "q3"]
    tsize = {"tA": 9000, "tB": 7000, "t10": 8000}
    contigs = {q: b["q_pool"].tobytes() for q in qnames}
    for t in tnames:
        contigs[t] = pc.rand_seq(rng, tsize[t], b"ACGTacgtN")
    recs, cursor = [], {}
    for i in range(36):
        t, q = tnames[i % 3], qnames[(i // 3) % 3]
        cur = cursor.get((t, q), 0)
        mode = rng.integers(0, 4)   # gap / abut / partial overlap / contained
        start = cur + int(rng.integers(1, 60)) if mode == 0 or cur == 0 else \
            cur if mode == 1 else max(0, cur - int(rng.integers(1, 40))) if mode == 2 else max(0, cur - int(tspan[i]) - 5)
        end = start + int(tspan[i])
        if end > tsize[t]:
            continue
        cursor[(t, q)] = max(cur, end)
        qs = int(b["q_src_off"][i])
        recs.append(dict(tname=t, qname=q, tlen=tsize[t], tstart=start, tend=end, qlen=len(b["q_pool"]),
                         qstart=qs, qend=qs + int(b["q_src_len"][i]), strand="-" if b["strand_neg"][i] else "+",
                         cg=pc.rec_text(b, i)))
    rng.shuffle(recs)
    paf = tmp_path / "all.paf"
    paf.write_text(paf_text(recs))
    fa = tmp_path / "all.fa"
    fa.write_bytes(fasta_text(contigs))
    return paf, (fa if base else None), recs, contigs


WINDOW_BYTES = (1, 300, 4096, 20000)     # every line a window of its own ... several lines per window


def check_cli_parity(cli, tmp_path, base):
    """the device writer at the default window, at four small ones, and the host writer: the same files, which are the
    reference's rows; WGA_TIMING names the writer that ran"""
    import cli_cases as cc
    paf, fa, recs, contigs = end_to_end_input(tmp_path, base)
    exp = cc._expected_pseudo_files(recs, contigs, base)
    rc, msg, timing, dev = pafpseudo(cli, tmp_path, "dev", paf, fa)
    assert rc == 0, msg
    assert "pafpseudo rows (device)" in timing and "pafpseudo rows (host)" not in timing, timing
    rc, msg, timing, host = pafpseudo(cli, tmp_path, "host", paf, fa, env=HOST_WRITER)
    assert rc == 0, msg
    assert "pafpseudo rows (host)" in timing and "pafpseudo rows (device)" not in timing, timing
    assert sorted(dev) == sorted(t + ".maf" for t in exp)
    assert dev == host
    for t, text in exp.items():
        got = dev[t + ".maf"]
        # the reference writes query rows in HashMap order: compare rows as a multiset, header first
        assert got.split(b"\n")[:2] == text.split(b"\n")[:2]
        assert sorted(got.split(b"\n")) == sorted(text.split(b"\n")), t
    for w in WINDOW_BYTES:
        rc, msg, timing, got = pafpseudo(cli, tmp_path, "dev_%d" % w, paf, fa, env={"WGA_PSEUDO_OUT_BYTES": str(w)})
        assert rc == 0, (w, msg)
        assert "pafpseudo rows (device)" in timing
        assert got == dev, w


def geometry_recs():
    def rec(q, t, tlen, ts, te, cg, strand="+"):
        return dict(tname=t, qname=q, tlen=tlen, tstart=ts, tend=te, qlen=1000, qstart=0, qend=te - ts, strand=strand, cg=cg)
    return [rec("q1", "tA", 500, 10, 110, "cg:Z:100="),
            rec("q2", "tA", 500, 100, 500, "cg:Z:200=10X190="),           # ends at the target's size: a tail of 0
            rec("q1", "tA", 500, 140, 200, "cg:Z:60=", "-"),              # overlaps the record in front by 10 columns
            rec("q1", "tA", 500, 110, 150, "cg:Z:30=5X5="),               # abuts [10, 110): a gap of 0
            rec("q1", "tA", 500, 150, 180, "xx:i:0"),                     # contained in [140, 200): dropped, never tokenised or filled
            rec("q1", "tA", 500, 260, 285, "cg:Z:10=5D10="),
            rec("q3", "tB", 200, 0, 200, "cg:Z:200=")]                    # a target of one record, no gap and no tail


def check_cli_geometry(cli, tmp_path):
    """abutting, overlapping and contained segments, a row without a tail, a target of one record; `-g`; the host reader's
    records under the device writer"""
    import cli_cases as cc
    recs = geometry_recs()
    exp = cc._expected_pseudo_files(recs, {}, False)
    assert exp["tA"].count(b"\n") == 5 and b"\t" + b"1" * 200 + b"\n" in exp["tB"]
    paf = tmp_path / "geo.paf"
    paf.write_text(paf_text(recs))
    want = {t + ".maf": text for t, text in exp.items()}         # one query after the other as they first appear: the same bytes
    runs = {"dev": {}, "dev_64": {"WGA_PSEUDO_OUT_BYTES": "64"}, "dev_1": {"WGA_PSEUDO_OUT_BYTES": "1"}, "host": HOST_WRITER,
            "dev_host_reader": {"WGA_PAF_READER": "host"}, "dev_host_reader_64": {"WGA_PAF_READER": "host", "WGA_PSEUDO_OUT_BYTES": "64"}}
    for name, env in runs.items():
        rc, msg, timing, got = pafpseudo(cli, tmp_path, name, paf, env=env)
        assert rc == 0, (name, msg)
        assert ("pafpseudo rows (host)" if name == "host" else "pafpseudo rows (device)") in timing, (name, timing)
        assert got == want, name
    rc, msg, _, got = pafpseudo(cli, tmp_path, "only_tB", paf, extra=["-g", "tB"])
    assert rc == 0 and got == {"tB.maf": want["tB.maf"]}, msg
    rc, msg, _, got = pafpseudo(cli, tmp_path, "only_tB", paf, extra=["-g", "tB"])             # the directory rule is as it was
    assert rc == 1 and "already exists" in msg
    rc, msg, _, got = pafpseudo(cli, tmp_path, "only_tB", paf, extra=["-r", "-g", "tA"])
    assert rc == 0 and got == want, msg


def check_cli_errors(cli, tmp_path):
    """what only a window's fill finds — an invalid base on a `-` strand record of the second target, a query slice shorter than
    its CIGAR consumes — ends the run with the host writer's message; the first target's file is complete by then"""
    rng = np.random.default_rng(11)
    lut = np.frombuffer(b"ACGT", dtype=np.uint8)
    q1 = bytearray(lut[rng.integers(0, 4, 200)].tobytes())
    q1[150] = ord("R")
    contigs = {"q1": bytes(q1), "tA": lut[rng.integers(0, 4, 300)].tobytes(), "tB": lut[rng.integers(0, 4, 300)].tobytes()}
    fa = tmp_path / "err.fa"
    fa.write_bytes(fasta_text(contigs))

    def rec(t, ts, te, qs, qe, cg, strand="+"):
        return dict(tname=t, qname="q1", tlen=300, tstart=ts, tend=te, qlen=200, qstart=qs, qend=qe, strand=strand, cg=cg)
    first = [rec("tA", 10, 110, 0, 100, "cg:Z:100="), rec("tB", 0, 50, 0, 50, "cg:Z:50=")]
    cases = {"base": (rec("tB", 100, 160, 120, 180, "cg:Z:60=", "-"), "Invalid Base: `R`"),
             "drain": (rec("tB", 100, 125, 0, 30, "cg:Z:20=20I5="), "panic: String::drain / insert_str beyond the end of the query")}
    for name, (bad, want_msg) in cases.items():
        paf = tmp_path / (name + ".paf")
        paf.write_text(paf_text(first + [bad]))
        rc, host_msg, _, host_files = pafpseudo(cli, tmp_path, name + "_host", paf, fa, env=HOST_WRITER)
        assert rc == 1 and want_msg in host_msg, host_msg
        rc, _, _, only_a = pafpseudo(cli, tmp_path, name + "_host_tA", paf, fa, env=HOST_WRITER, extra=["-g", "tA"])
        assert rc == 0 and list(only_a) == ["tA.maf"] and only_a["tA.maf"].count(b"\n") == 4
        for w in ("default", "64"):
            env = {} if w == "default" else {"WGA_PSEUDO_OUT_BYTES": w}
            rc, msg, timing, got = pafpseudo(cli, tmp_path, "%s_dev_%s" % (name, w), paf, fa, env=env)
            assert rc == 1 and msg == host_msg, (name, w, msg, host_msg)
            assert "pafpseudo rows (device)" in timing
            assert got["tA.maf"] == only_a["tA.maf"], (name, w)
            whole = b"a score=0\ns\ttB\t0\t300\t+\t300\t" + contigs["tB"] + b"\n"
            assert got["tB.maf"] == (b"" if w == "default" else whole), (name, w, got["tB.maf"][:80])   # it ends at the last window written


def check_cli_gpus(cli, tmp_path, gpus=2):
    """--gpus N: every device runs its own targets' windows; the files of one device"""
    for base in (False, True):
        sub = tmp_path / ("base" if base else "sym")
        sub.mkdir()
        paf, fa, recs, contigs = end_to_end_input(sub, base)
        rc, msg, _, one = pafpseudo(cli, sub, "one", paf, fa, env={"WGA_PSEUDO_OUT_BYTES": "4096"})
        assert rc == 0 and len(one) == 3, msg
        import maf2paf_cases as m2p
        outdir = sub / "gpus"
        args = ["--gpus", str(gpus), "pafpseudo", str(paf), "-o", str(outdir)] + (["-f", str(fa)] if fa else [])
        rc, _, msg, timing = m2p.timed(cli, args, {"WGA_PSEUDO_OUT_BYTES": "4096"})
        assert rc == 0, msg
        assert "pafpseudo rows (device)" in timing
        assert {f: open(outdir / f, "rb").read() for f in sorted(os.listdir(outdir))} == one
