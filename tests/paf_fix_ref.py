"""`validate` and `validate --fix` restated in plain Python from the file's bytes (tools/validate.rs:44-141 with the csv writer of
parser/paf.rs:50-65): parse every record, sum its CIGAR, print.  For plain PAF text only — no quoted field, no CR: a line is
split at its tabs and the nine numbers are parsed and printed again, so `007` and `+5` come out as `7` and `5` as the csv
writer's do.  Independent of how the device finds a column: the fields come from bytes.split."""
import re

U64 = (1 << 64) - 1
NUM_COLS = (1, 2, 3, 6, 7, 8, 9, 10, 11)


class InvalidOp(Exception):
    pass


def cigar_sums(cg):
    """(query bases, target bases) of a CIGAR text: M = X and I on the query, M = X and D on the target (cigar.rs:638-700)"""
    ops = re.findall(rb"(\d+)([A-Za-z=])", cg)
    assert b"".join(n + o for n, o in ops) == cg and ops, cg[:80]
    q = t = 0
    for n, o in ops:
        n = int(n)
        if o in b"M=X":
            q, t = q + n, t + n
        elif o == b"I":
            q += n
        elif o == b"D":
            t += n
        else:
            raise InvalidOp(o.decode())
    return q & U64, t & U64


def records(data):
    """the fields of every record line: blank lines and `#` lines are dropped (the csv reader's comment rule)"""
    lines = data.split(b"\n")
    if lines and lines[-1] == b"":
        lines.pop()
    return [ln.split(b"\t") for ln in lines if ln and not ln.startswith(b"#")]


def cigar_of(f):
    for tag in f[12:]:
        if tag.startswith(b"cg:Z:"):
            return tag[5:]
    raise KeyError("no cg:Z: tag")


def fix(data):
    """(rows, qlist, tlist, n_records, n_q_bad, n_t_bad)"""
    rows, ql, tl = [], [], []
    recs = records(data)
    for f in recs:
        f = list(f)
        for c in NUM_COLS:
            f[c] = b"%d" % int(f[c])
        dq, dt = cigar_sums(cigar_of(f))
        eq, et = (int(f[2]) + dq) & U64, (int(f[7]) + dt) & U64
        if eq != int(f[3]):
            ql.append(b"%s:%s-%s\n" % (f[0], f[2], f[3]))
            f[3] = b"%d" % eq
        if et != int(f[8]):
            tl.append(b"%s:%s-%s\n" % (f[5], f[7], f[8]))
            f[8] = b"%d" % et
        rows.append(b"\t".join(f) + b"\n")
    return b"".join(rows), b"".join(ql), b"".join(tl), len(recs), len(ql), len(tl)


def report(data):
    """what `validate` writes to its output in front of the fixed rows"""
    rows, ql, tl, n, nq, nt = fix(data)
    return (b"Total records: %d\nQuery invalid records: %d\nTarget invalid records: %d\nQuery invalid list:\n" % (n, nq, nt) + ql +
            b"Target invalid list:\n" + tl + b"\n")
