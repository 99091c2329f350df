"""`chain2paf` restated in plain Python from the chain splitter's arrays: what wga_chain2paf (K27) has to write for (heads,
triples, line_off, text).  Written from convert2paf (chain.rs:430-452), parse_chain_to_cigar (cigar.rs:554-627) and the rule of
the csv writer that prints the record (tab delimiter, QuoteStyle::Necessary)."""

U64 = (1 << 64) - 1


def csv_field(name):
    """as it is, unless it holds the delimiter, a quote, CR or LF; then between quotes, every quote inside doubled"""
    if not any(c in name for c in (b"\t", b'"', b"\n", b"\r")):
        return name
    return b'"' + name.replace(b'"', b'""') + b'"'


def cigar_and_sums(rows):
    """(cg text, matches, block_length) of a chain's data lines (size, col2, col3): `<size>M` always, col3 as I and col2 as D when
    non-zero; matches = the sizes, block_length = matches + mismatch (0) + del + inv_del (= the 2nd columns on either strand),
    as the u64 columns of the record: mod 2^64"""
    cg, matches, dels = [], 0, 0
    for size, col2, col3 in rows:
        cg.append(b"%dM" % size)
        if col3:
            cg.append(b"%dI" % col3)
        if col2:
            cg.append(b"%dD" % col2)
        matches += size
        dels += col2
    return b"".join(cg), matches & U64, (matches + dels) & U64


def record(head, rows, text):
    num = [int(v) for v in head["num"]]
    tname = text[int(head["tname_off"]):int(head["tname_off"]) + int(head["tname_len"])]
    qname = text[int(head["qname_off"]):int(head["qname_off"]) + int(head["qname_len"])]
    cg, matches, block = cigar_and_sums(rows)
    cols = [csv_field(qname), b"%d" % num[4], b"%d" % num[5], b"%d" % num[6], b"-" if head["qstrand_neg"] else b"+",
            csv_field(tname), b"%d" % num[1], b"%d" % num[2], b"%d" % num[3], b"%d" % matches, b"%d" % block, b"255", b"cg:Z:" + cg]
    return b"\t".join(cols) + b"\n"


def chain2paf_ref(heads, triples, line_off, text):
    """the text of all records"""
    out = []
    for r, h in enumerate(heads):
        rows = [tuple(int(v) for v in triples[l]) for l in range(int(line_off[r]), int(line_off[r + 1]))]
        out.append(record(h, rows, text))
    return b"".join(out)
