"""The frame of a MAF record as `paf2maf` and `chain2maf` write it, restated in Python integers from the reference's behaviour
(MAFWriter::write_record, maf.rs:566-581, behind converter.rs:196-263 and :288-355), and the layout of a batch of records.
The expectation of the K32 tests (maf_frame_cases.py); no code of the project is used here."""
U64 = (1 << 64) - 1


def s_line(name, nums, neg):
    """the head of an `s` line up to the tab in front of the row; nums = (start, aligned size, source size) as printed"""
    return b"s\t%s\t%d\t%d\t%s\t%d\t" % (name, nums[0] & U64, nums[1] & U64, b"-" if neg else b"+", nums[2] & U64)


def t_head(score, name, nums, neg):
    """the `a` line and the head of the target's `s` line: what stands in front of the target row"""
    return b"a score=%d\n" % (score & U64) + s_line(name, nums, neg)


def q_head(name, nums, neg):
    """the end of the target's line and the head of the query's `s` line: what stands between the two rows"""
    return b"\n" + s_line(name, nums, neg)


TAIL = b"\n\n"                                                                    # the end of the query's line, the blank line


def layout(t_heads, t_rows, q_heads, q_rows):
    """(t_row_off, q_row_off, rec_off with the text's length last) of records that stand back to back: the byte counts of
    the heads and the rows in, places out, all in Python integers"""
    t_off, q_off, rec_off, at = [], [], [], 0
    for th, tr, qh, qr in zip(t_heads, t_rows, q_heads, q_rows):
        rec_off.append(at)
        t_off.append(at + th)
        q_off.append(at + th + tr + qh)
        at += th + tr + qh + qr + len(TAIL)
    return t_off, q_off, rec_off + [at]


def n_good(diags):
    """the first record with a diagnostic; diags = (bad_op_idx, panic_op_idx, bad_base_pos) per record, U64 = not set"""
    for r, g in enumerate(diags):
        if any(v != U64 for v in g):
            return r
    return len(diags)
