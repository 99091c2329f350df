"""An independent restatement of `wgatools filter` (tools/filter.rs, utils.rs:540-576) on MAF, PAF and chain and of `wgatools
rename` (tools/rename.rs, MAFRecord::rename maf.rs:250-261) with the record writer (maf.rs:566-581): the tests' expectation.
Written from the reference's behaviour; nothing here is shared with the C++.

MAF blocks are those of maf_chunk_ref.read_blocks: [(name, start, size, strand, src_size, seq), ...] per block.  The writer
prints the parsed u64 fields in decimal (an input `007` leaves as `7`); `size` is the field, not a count of the text."""
from decimal import Decimal

U64 = (1 << 64) - 1


# ---- MAF ---------------------------------------------------------------------------------------------------------------------
def record(rows, prefixes=None):
    out = [b"a score=255\n"]
    for i, (name, start, size, strand, src, seq) in enumerate(rows):
        out.append(b"s\t%s%s\t%d\t%d\t%s\t%d\t%s\n" % (prefixes[i] if prefixes else b"", name, start, size, strand, src, seq))
    out.append(b"\n")
    return b"".join(out)


def filter_header(b, q):
    return b"#maf version=1.6 filter=blocksize>=%d querysize>=%d\n" % (b, q)


def rename_header(prefixes):
    return b"#maf version=1.6 rename=%s\n" % b";".join(prefixes)


def filter_maf(blocks, b, q):
    """(text, bad): the kept blocks' records; bad = the index of the first block with fewer than two rows (query_length()
    indexes slines[1] before anything is compared: the text ends in front of it), None otherwise"""
    out = []
    for i, rows in enumerate(blocks):
        if len(rows) < 2:
            return b"".join(out), i
        query_length, block_length = rows[1][4], rows[0][2]
        if block_length < b or query_length < q:
            continue
        out.append(record(rows))
    return b"".join(out), None


def rename_maf(blocks, prefixes):
    """(text, bad): bad = the first block whose row count differs from the number of prefixes"""
    out = []
    for i, rows in enumerate(blocks):
        if len(rows) != len(prefixes):
            return b"".join(out), i
        out.append(record(rows, prefixes))
    return b"".join(out), None


def sizes_agree(blocks):
    """every size field equals its row's bytes that are not '-' (then `filter` at thresholds 0 writes what `chunk` with one
    chunk per block writes)"""
    return all(size == len(seq) - seq.count(b"-") for rows in blocks for (_n, _s, size, _st, _src, seq) in rows)


# ---- PAF (csv crate reader: tab, flexible, '#' comments; writer QuoteStyle::Necessary) ------------------------------------------
def csv_records(text):
    """the records of a tab-separated text: they end at \\n, \\r\\n or \\r; empty lines and lines that start with '#' are
    skipped; a field that starts with '"' is quoted ('""' is a quote), what follows its closing quote is kept as it is"""
    recs, i, n = [], 0, len(text)
    while i < n:
        if text[i:i + 1] in (b"\n", b"\r"):
            i += 1
            continue
        if text[i:i + 1] == b"#":
            while i < n and text[i:i + 1] not in (b"\n", b"\r"):
                i += 1
            continue
        fields, cur = [], bytearray()
        start = True
        while True:
            if i >= n or text[i:i + 1] in (b"\n", b"\r"):
                fields.append(bytes(cur))
                break
            ch = text[i:i + 1]
            if ch == b"\t":
                fields.append(bytes(cur))
                cur, start = bytearray(), True
                i += 1
                continue
            if start and ch == b'"':
                i += 1
                while i < n:
                    if text[i:i + 1] == b'"':
                        if text[i + 1:i + 2] == b'"':
                            cur += b'"'
                            i += 2
                            continue
                        i += 1
                        break
                    cur += text[i:i + 1]
                    i += 1
                start = False
                continue
            cur += ch
            start = False
            i += 1
        recs.append(fields)
    return recs


def csv_field(f):
    if any(c in f for c in (b"\t", b'"', b"\n", b"\r")):
        return b'"' + f.replace(b'"', b'""') + b'"'
    return f


def paf_row(f):
    """PafRecord's field order (paf.rs:50-65): the twelve fixed fields with the numbers re-printed, then every tag"""
    nums = {1, 2, 3, 6, 7, 8, 9, 10, 11}
    return b"\t".join(b"%d" % int(x) if k in nums else csv_field(x) for k, x in enumerate(f)) + b"\n"


def filter_paf(text, b, q):
    out = []
    for f in csv_records(text):
        block_length = (int(f[8]) - int(f[7])) & U64
        if block_length < b or int(f[1]) < q:
            continue
        out.append(paf_row(f))
    return b"".join(out)


PAF_ALIGN_WARNING = "`min_align_size` is set, will not filter paf `min_block_size` and `min_query_size`"


def filter_paf_pairs(text, a):
    recs = csv_records(text)
    total = {}
    for f in recs:
        key = (f[0], f[5])
        total[key] = (total.get(key, 0) + ((int(f[8]) - int(f[7])) & U64)) & U64
    return b"".join(paf_row(f) for f in recs if total[(f[0], f[5])] >= a)


# ---- chain ---------------------------------------------------------------------------------------------------------------------
def f64_display(text):
    """Rust's Display of the f64 that `text` parses to: the shortest digits that read back as the same value, positional,
    never an exponent, no trailing `.0`"""
    s = format(Decimal(repr(float(text))), "f")
    if "." in s:
        s = s.rstrip("0").rstrip(".")
    return s


def filter_chain(text, b, q):
    """well-formed chains only: a header line of twelve fields behind `chain`, data lines of one to three numbers, then
    anything up to the next `c`"""
    out, lines, i = [], text.split(b"\n"), 0
    while i < len(lines):
        if not lines[i].startswith(b"chain"):
            i += 1
            continue
        h = lines[i][5:].split()
        i += 1
        data = []
        while i < len(lines) and lines[i] and not any(c in lines[i] for c in b"chain"):
            v = [int(x) for x in lines[i].split()[:3]]
            data.append(v + [0] * (3 - len(v)))
            i += 1
        if (int(h[5]) - int(h[4])) & U64 < b or int(h[7]) < q:
            continue
        out.append(b"chain\t" + f64_display(h[0].decode()).encode() + b"\t" + b"\t".join(
            b"%d" % int(x) if k in (1, 3, 4, 6, 8, 9, 10) else x for k, x in enumerate(h[1:12])))
        for v in data:
            out.append(b"\n%d\t%d\t%d" % tuple(v))
        out.append(b"\n\n")
    return b"".join(out)
