"""`maf2paf` restated in plain Python from the arrays wga_maf2paf (K28) takes: what it has to write for (heads, counts, runs,
run_off, cols, names).  Written from the record of maf.rs:484-520 (the twelve columns, `NM:i:` and the `cg:Z:` text of the column
classes) and the rule of the csv writer that prints it (converter.rs:29-54: tab delimiter, QuoteStyle::Necessary)."""

U64 = (1 << 64) - 1
LETTERS = "=IDXXXXX"


def csv_field(name):
    """as it is, unless it holds the delimiter, a quote, CR or LF; then between quotes, every quote inside doubled"""
    if not any(c in name for c in (b"\t", b'"', b"\n", b"\r")):
        return name
    return b'"' + name.replace(b'"', b'""') + b'"'


def cigar(runs, lo, hi, cols_r):
    """the cg:Z: text of runs[lo:hi] (start column << 3 | class): a run's length is the next run's start, or the block's columns
    behind the last, minus its own start (mod 2^64); the letter is its class"""
    out = []
    for x in range(lo, hi):
        start = int(runs[x]) >> 3
        end = int(runs[x + 1]) >> 3 if x + 1 < hi else int(cols_r)
        out.append("%d%s" % ((end - start) & U64, LETTERS[int(runs[x]) & 7]))
    return "".join(out).encode()


def name_of(names, off, length):
    off, length = int(off), int(length)
    return names[off:off + length] if off <= len(names) and length <= len(names) - off else b""


def record(head, cnt, cg, names):
    matches = int(cnt["match"])
    block = sum(int(cnt[k]) for k in ("match", "mismatch", "ins_bp", "inv_ins_bp", "del_bp", "inv_del_bp")) & U64
    q, t = [int(v) for v in head["q"]], [int(v) for v in head["t"]]
    cols = [csv_field(name_of(names, head["qname_off"], head["qname_len"])), b"%d" % q[0], b"%d" % q[1], b"%d" % q[2],
            b"-" if head["strand_neg"] else b"+", csv_field(name_of(names, head["tname_off"], head["tname_len"])),
            b"%d" % t[0], b"%d" % t[1], b"%d" % t[2], b"%d" % matches, b"%d" % block, b"255",
            b"NM:i:%d" % ((block - matches) & U64), b"cg:Z:" + cg]
    return b"\t".join(cols) + b"\n"


def maf2paf_ref(heads, counts, runs, run_off, cols, names):
    """the text of all records"""
    return b"".join(record(heads[r], counts[r], cigar(runs, int(run_off[r]), int(run_off[r + 1]), cols[r]), names)
                    for r in range(len(heads)))
