"""The base-level csv rows of `dotplot` restated in plain Python from the format of include/wga_hip.h (K26), not from the kernel:
for every segment `<s0>,<s1>,<s2>,<s3>,<M|I|D>` and then the tail of the segment's record; plus the csv quoting that makes a tail
(the rule of the host's append_csv_field: a field with the delimiter, a quote, LF or CR is wrapped in quotes, its quotes doubled)."""


def csv_field(name, delim=b","):
    if any(c in name for c in (delim, b'"', b"\n", b"\r")):
        return b'"' + name.replace(b'"', b'""') + b'"'
    return name


def tail(ref_chro, query_chro):
    return b"," + csv_field(ref_chro) + b"," + csv_field(query_chro) + b"\n"


def rows_ref(segs, seg_off, tails):
    """segs: rows of five ints; seg_off: n + 1 ascending ints; tails: n byte strings.  A kind above 2 prints `?`"""
    out = []
    for rec in range(len(tails)):
        for x in range(int(seg_off[rec]), int(seg_off[rec + 1])):
            s = [int(v) for v in segs[x]]
            out.append(b"%d,%d,%d,%d,%c" % (s[0], s[1], s[2], s[3], b"MID"[s[4]] if s[4] < 3 else ord("?")) + tails[rec])
    return b"".join(out)
