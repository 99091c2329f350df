"""What `stat` prints without --each, restated from the reference (merge_final_from_pair stat.rs:167-223 through the csv writer of
stat.rs:117-123) — independently of the kernels and of the host's stat_tsv:
  * the pairs stand in first-appearance order (the reference walks a HashMap, whose order is random; the sort by natord of ref_name
    that follows is stable, so first appearance is the order this project fixes);
  * the eleven counters and aligned_size are summed mod 2^64, the two starts are minima that begin at the sizes;
  * inv_size is the sum of the records' numpy.float32 values, added one by one in record order into a numpy.float32;
  * the row text, csv quoting and natord's order are stat_rows_ref's."""
import functools

import numpy as np

import stat_rows_ref as rows_ref

U64 = (1 << 64) - 1
COUNT_FIELDS = rows_ref.COUNT_FIELDS
HEADER = rows_ref.HEADER


def as_counts(c):
    return c if isinstance(c, dict) else dict(zip(COUNT_FIELDS, (int(v) for v in c)))


def f32_bits(x):
    return int(np.array([x], dtype=np.float32).view(np.uint32)[0])


def inv_size(c):
    """a record's f32 inv_size (common.rs:116-140): +0.0 without an inversion"""
    return rows_ref.floats(c)[3]


def pairs(records, inv_in=None):
    """records = [(ref_name, ref_size, ref_start, query_name, query_size, query_start, counts)] (names as bytes).  Returns
    (the pairs in first-appearance order, pair_of_rec); a pair is a dict with key (ref_name, ref_size, query_name, query_size),
    first_rec, n_recs, ref_start, query_start, sum (a dict over COUNT_FIELDS) and inv_size (numpy.float32).
    inv_in: the start values of the inv_size sums by pair number, as f32 bit patterns"""
    index, out, pair_of_rec = {}, [], []
    for k, (rn, rs, rst, qn, qs, qst, c) in enumerate(records):
        c = as_counts(c)
        key = (bytes(rn), int(rs), bytes(qn), int(qs))
        if key not in index:
            index[key] = len(out)
            start = np.float32(0) if inv_in is None else rows_ref.f32_of_bits(int(inv_in[len(out)]))
            out.append(dict(key=key, first_rec=k, n_recs=0, ref_start=int(rs), query_start=int(qs), sum=dict.fromkeys(COUNT_FIELDS, 0),
                            inv_size=start))
        p = out[index[key]]
        pair_of_rec.append(index[key])
        p["n_recs"] += 1
        for f in COUNT_FIELDS:
            p["sum"][f] = (p["sum"][f] + c[f]) & U64
        with np.errstate(over="ignore", invalid="ignore"):
            p["inv_size"] = np.float32(p["inv_size"] + inv_size(c))
        p["ref_start"] = min(p["ref_start"], int(rst))
        p["query_start"] = min(p["query_start"], int(qst))
    return out, pair_of_rec


def pair_row(ref_name, ref_size, ref_start, query_name, query_size, query_start, s, inv):
    """the row of a pair: s = the summed counters, inv = its inv_size (numpy.float32)"""
    s = as_counts(s)
    aligned, identity, similarity, _ = rows_ref.floats(dict(s, inv_ev=0))
    cols = [rows_ref.csv_field(ref_name), b"%d" % ref_size, b"%d" % ref_start, rows_ref.csv_field(query_name), b"%d" % query_size,
            b"%d" % query_start, b"%d" % aligned, b"%d" % ((ref_size - aligned) & U64), rows_ref.f32_text(identity),
            rows_ref.f32_text(similarity)]
    cols += [b"%d" % s[k] for k in ("match", "mismatch", "ins_ev", "del_ev", "ins_bp", "del_bp", "inv_ev")]
    cols.append(rows_ref.f32_text(inv))
    cols += [b"%d" % s[k] for k in ("inv_ins_ev", "inv_ins_bp", "inv_del_ev", "inv_del_bp")]
    return b"\t".join(cols) + b"\n"


def row_of(p):
    rn, rs, qn, qs = p["key"]
    return pair_row(rn, rs, p["ref_start"], qn, qs, p["query_start"], p["sum"], p["inv_size"])


def table(records):
    """the whole output: the header and the pairs' rows sorted stably by natord of ref_name, or nothing without a record"""
    if not records:
        return b""
    ps, _ = pairs(records)
    names = [p["key"][0].decode("utf-8", "replace") for p in ps]
    order = sorted(range(len(ps)), key=functools.cmp_to_key(lambda x, y: rows_ref.natord_compare(names[x], names[y])))
    return HEADER + b"".join(row_of(ps[k]) for k in order)
