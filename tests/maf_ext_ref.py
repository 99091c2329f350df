"""A naive restatement of `wgatools maf-index` (tools/index.rs:14-94, utils.rs:334-350) and `wgatools maf-ext`
(tools/mafextra.rs:25-232, utils.rs:353-394) over raw file bytes: the tests' expectation.

Reader (maf.rs:25-36, 371-421): the first line is the header; a record is a maximal run of lines that start with `s`; the
line that ends the run is consumed with it; every other line in front of a run is skipped.  index.rs:22 takes the stream
position in front of every `records().next()`: a block's offset is the position just behind the line that ended the record
in front of it (behind the header line for the first block), so the skipped lines in front of its first `s` line lie inside
its span.

Hits (mafextra.rs:176-180): rust-lapper 1.1.0.  `Lapper::new` sorts the intervals with `sort()` (stable) by the `Ord` of
`Interval`, which compares `start`, then `stop`, and not `val` (the offset); `find(start, stop)` yields, in that order, the
intervals with `iv.start < stop && iv.stop > start`.  The crate's source is not at hand here: this is its documented
behaviour, stated so that it can be challenged."""
import functools

import numpy as np


def _lines(data, pos):
    """(start, end behind the line feed, text without the line end) of every line from pos on (BufRead::lines)"""
    n = len(data)
    while pos < n:
        e = data.find(b"\n", pos)
        end = n if e < 0 else e + 1
        ln = data[pos:end]
        if ln.endswith(b"\n"):
            ln = ln[:-1]
            if ln.endswith(b"\r"):
                ln = ln[:-1]
        yield pos, end, ln
        pos = end


def _sline(ln):
    f = ln.split()
    if not (len(f) == 7 and f[2].isdigit() and f[3].isdigit() and f[5].isdigit() and f[4] in (b"+", b"-")):
        raise ValueError("bad s-line")
    return (f[1], int(f[2]), int(f[3]), f[4], int(f[5]), f[6])


def header_end(data):
    e = data.find(b"\n")
    return len(data) if e < 0 else e + 1


def record_at(data, pos):
    """MAFRecords::next (maf.rs:371-421) from byte pos: (rows, position behind the line that ended the record) or None"""
    rows = None
    for _s, end, ln in _lines(data, pos):
        if ln[:1] == b"s":
            rows = (rows or []) + [_sline(ln)]
            pos = end
        elif rows is None:
            pos = end           # maf.rs:382-383: skipped
        else:
            return rows, end    # maf.rs:409-411: the line that ends the run is consumed
    return (rows, pos) if rows is not None else None


def blocks_with_offsets(data):
    """[(offset, rows)] as index.rs:21-28 sees them"""
    out, pos = [], header_end(data)
    while True:
        rec = record_at(data, pos)
        if rec is None:
            return out
        out.append((pos, rec[0]))
        pos = rec[1]


def build_index(data):
    """(index, error): index.rs:30-68 — name -> {"ivls": [...], "size", "isref"} in order of first appearance"""
    idx = {}
    for offset, rows in blocks_with_offsets(data):
        seen = []
        for ord_, (name, start, asize, strand, size, _seq) in enumerate(rows):
            if name in seen:                                                              # index.rs:33-37
                return None, "Duplicate name `%s` in a record not allowed, please check or use `rename`" % name.decode()
            seen.append(name)
            key = name.decode("utf-8", "surrogateescape")
            if key not in idx:
                idx[key] = {"ivls": [], "size": size, "isref": ord_ == 0}                 # index.rs:44-53
            elif idx[key]["isref"] != (ord_ == 0):                                        # index.rs:54-58
                return None, "Same sequence cannot be both reference and query!"
            idx[key]["ivls"].append({"start": start, "end": start + asize, "strand": strand.decode(), "offset": offset})
    if not idx:
        return None, "Empty record"                                                       # index.rs:71-75
    return idx, None


def ref_contigs(index):
    """the (name, size) of the isref entries, as `call` writes its ##contig lines (natural order is the caller's business)"""
    return [(k, v["size"]) for k, v in index.items() if v["isref"]]


def find_hits(ivls, g_start, g_end):
    """the lapper rule of the module docstring"""
    order = sorted(range(len(ivls)), key=lambda i: (ivls[i]["start"], ivls[i]["end"]))    # stable
    return [ivls[i] for i in order if ivls[i]["start"] < g_end and ivls[i]["end"] > g_start]


@functools.lru_cache(maxsize=8)
def _ascii_base_columns(seq):
    return np.flatnonzero(np.frombuffer(seq, dtype=np.uint8) != 0x2D)


def col_coord(seq, pos):
    """get_col_coord (maf.rs:81-95): the CHARACTER index of the pos-th non-gap character, the BYTE length when there is none"""
    if len(seq) > 100000 and seq.isascii():      # the same walk for a long ASCII row (character = byte), vectorised
        cols = _ascii_base_columns(seq)
        return int(cols[pos]) if pos < len(cols) else len(seq)
    k = 0
    for i, ch in enumerate(seq.decode("utf-8", "replace")):
        if ch != "-":
            if k == pos:
                return i
            k += 1
    return len(seq)


class Panic(Exception):
    pass


def _str_slice(seq, a, b):
    """&seq[a..b] of a Rust String: byte indices, panics outside the string or inside a character"""
    if a > b or b > len(seq):
        raise Panic("slice index out of range")
    for x in (a, b):
        if x < len(seq) and (seq[x] & 0xC0) == 0x80:
            raise Panic("byte index is not a char boundary")
    return seq[a:b]


def record_text(rows):
    """maf.rs:566-581"""
    return b"a score=255\n" + b"".join(b"s\t%s\t%d\t%d\t%s\t%d\t%s\n" % r for r in rows) + b"\n"


def slice_rows(rows, cut_start, cut_end, ord_):
    """slice_block (maf.rs:223-248)"""
    name, start, _asize, strand, size, seq = rows[ord_]
    if cut_start < start:
        raise ValueError("the index does not belong to this file")
    lo, hi = cut_start - start, cut_end - start                                          # maf.rs:226-227
    c0, c1 = col_coord(seq, lo), col_coord(seq, hi)                                       # maf.rs:232-233
    out = list(rows)
    out[ord_] = (name, cut_start, cut_end - cut_start, strand, size, _str_slice(seq, c0, c1))   # maf.rs:229-234
    for i, (n2, s2, _a2, st2, z2, q2) in enumerate(rows):
        if i == ord_:
            continue
        piece = _str_slice(q2, c0, c1)                                                    # maf.rs:240
        out[i] = (n2, s2 + lo, (c1 - c0) - piece.count(b"-"), st2, z2, piece)             # maf.rs:238-243
    return out, (c0, c1)


def parse_region(r):
    import re
    m = re.match(rb"^([a-zA-Z0-9.@_#-]+):([0-9]+)-([0-9]+)$", r)
    if not m:
        raise ValueError("Parse Genome Region Error By: Region `%s` is match the format of `chr:start-end`" % r.decode())
    s, e = int(m.group(2)), int(m.group(3))
    if s > e:
        raise ValueError("Parse Genome Region Error By: Start `%d` is larger than end `%d`" % (s, e))
    return (m.group(1), s, e)


def extract(data, index, regions, tally=None):
    """(text with the header, failed regions, panic): mafextra.rs:167-232.  index = the parsed JSON; regions = [(name, start,
    end)].  tally (a dict) counts hits: sliced, whole, c1 at the row's length, ord > 0."""
    out, failed = [b"#maf version=1.6 cmd=maf_extract\n"], []
    t = tally if tally is not None else {}
    for k in ("hits", "sliced", "whole", "c1_at_end", "ord_gt0"):
        t.setdefault(k, 0)
    for (name, g_start, g_end) in regions:
        item = index.get(name.decode("utf-8", "surrogateescape"))
        hits = find_hits(item["ivls"], g_start, g_end) if item is not None else []
        if not hits:
            failed.append((name, g_start, g_end))                                         # mafextra.rs:181-184, 226-229
            continue
        for iv in hits:
            rows = record_at(data, iv["offset"])[0]
            ords = [i for i, r in enumerate(rows) if r[0] == name]
            if not ords:
                continue                                                                  # mafextra.rs:193-196
            t["hits"] += 1
            if g_start <= iv["start"] and g_end >= iv["end"]:                             # mafextra.rs:204-207
                out.append(record_text(rows))
                t["whole"] += 1
                continue
            try:
                cut, (c0, c1) = slice_rows(rows, max(iv["start"], g_start), min(iv["end"], g_end), ords[0])
            except Panic as e:
                return b"".join(out), failed, str(e)
            t["sliced"] += 1
            t["c1_at_end"] += c1 == len(rows[ords[0]][5])
            t["ord_gt0"] += ords[0] > 0
            out.append(record_text(cut))
    return b"".join(out), failed, None
