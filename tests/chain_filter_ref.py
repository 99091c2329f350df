"""`filter -f chain` restated in plain Python from the chain splitter's arrays: what wga_chain_filter (K25) has to write for
(heads, triples, line_off, text) and two thresholds (chain.rs:92-100,185-204 behind tools/filter.rs:91-105)."""

U64 = (1 << 64) - 1


def keeps(head, min_block, min_query):
    """filter.rs:96-101: both compare with `<`, the span wraps"""
    num = [int(v) for v in head["num"]]
    return not (((num[3] - num[2]) & U64) < min_block or num[4] < min_query)


def head_text(head, text):
    num = [int(v) for v in head["num"]]
    tname = text[int(head["tname_off"]):int(head["tname_off"]) + int(head["tname_len"])]
    qname = text[int(head["qname_off"]):int(head["qname_off"]) + int(head["qname_len"])]
    return b"\t".join([b"chain", b"%d" % num[0], tname, b"%d" % num[1], b"-" if head["tstrand_neg"] else b"+", b"%d" % num[2],
                       b"%d" % num[3], qname, b"%d" % num[4], b"-" if head["qstrand_neg"] else b"+", b"%d" % num[5], b"%d" % num[6],
                       b"%d" % num[7]])


def filter_ref(heads, triples, line_off, text, min_block=0, min_query=0):
    """(the text of the kept chains, their number)"""
    out, kept = [], 0
    for r, h in enumerate(heads):
        if not keeps(h, min_block, min_query):
            continue
        kept += 1
        out.append(head_text(h, text))
        for l in range(int(line_off[r]), int(line_off[r + 1])):
            out.append(b"\n%d\t%d\t%d" % tuple(int(v) for v in triples[l]))
        out.append(b"\n\n")
    return b"".join(out), kept
