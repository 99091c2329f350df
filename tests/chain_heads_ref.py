"""The chain head of `paf2chain` / `maf2chain` restated in plain Python from chain.rs (the TryFrom arithmetic of :103-183, the
Display of :185-203): what wga_chain_heads (K30) has to write for hand-built trims that no CIGAR gives.  u64 arithmetic is
`& U64`, as Rust's wrapping release build computes it."""
U64 = (1 << 64) - 1


def coords(q, t, neg, trim):
    """(ts, te, qs, qe) of a record with q / t = (size, start, end) before trimming and trim = (head_ins, head_del, tail_ins,
    tail_del); on the '-' strand the end is computed from the start that was just updated (chain.rs:136-137,177-178)"""
    head_ins, head_del, tail_ins, tail_del = trim
    ts, te = (t[1] + head_del) & U64, (t[2] - tail_del) & U64
    if not neg:
        return ts, te, (q[1] + head_ins) & U64, (q[2] - tail_ins) & U64
    qs = (q[0] - ((q[2] - head_ins) & U64)) & U64
    return ts, te, qs, (q[0] - ((qs + tail_ins) & U64)) & U64


def head(qname, q, tname, t, neg, trim, chain_id):
    ts, te, qs, qe = coords(q, t, neg, trim)
    return b"chain\t255\t%s\t%d\t+\t%d\t%d\t%s\t%d\t%s\t%d\t%d\t%d" % (tname, t[0], ts, te, qname, q[0], b"-" if neg else b"+", qs,
                                                                     qe, chain_id & U64)


def layout(heads, nbytes, n_good):
    """(data_off of the good records, total): record r is its head, nbytes[r] bytes of data lines and two line ends"""
    at, off = 0, []
    for r in range(n_good):
        off.append(at + len(heads[r]))
        at = off[-1] + int(nbytes[r]) + 2
    return off, at
