"""What `stat --each` prints, restated from the reference (split_final stat.rs:129-164 through the csv writer of stat.rs:117-123,
over the record statistics of common.rs:116-140) — independently of the kernel and of the host's stat_tsv:
  * the three f32 columns are computed with numpy.float32 (conversion to nearest even, IEEE division);
  * their digits are numpy's Dragon4 in unique mode (format_float_scientific), laid out by ryu's rules (pretty::format32);
  * csv quoting (QuoteStyle::Necessary, tab delimiter) and natord's order (natord 1.0.9, `compare`) are restated here.
test_abi_stat_rows.py checks f32_text against the binary's hidden `__fmt_f32` hook (std::to_chars) for the whole pattern list."""
import functools

import numpy as np

U64 = (1 << 64) - 1
HEADER = (b"ref_name\tref_size\tref_start\tquery_name\tquery_size\tquery_start\taligned_size\tunaligned_size\tidentity\tsimilarity\t"
          b"matched\tmismatched\tins_event\tdel_event\tins_size\tdel_size\tinv_event\tinv_size\tinv_ins_event\tinv_ins_size\t"
          b"inv_del_event\tinv_del_size\n")
COUNT_FIELDS = ("match", "mismatch", "ins_ev", "ins_bp", "del_ev", "del_bp", "inv_ins_ev", "inv_ins_bp", "inv_del_ev", "inv_del_bp",
                "inv_ev")


def f32_of_bits(bits):
    return np.array([bits], dtype=np.uint32).view(np.float32)[0]


def f32_text(x):
    """ryu::Buffer::format(f32): x a numpy.float32"""
    x = np.float32(x)
    if np.isnan(x):
        return b"NaN"
    if np.isinf(x):
        return b"-inf" if x < 0 else b"inf"
    sign = b"-" if np.signbit(x) else b""
    if x == 0:
        return sign + b"0.0"
    sci = np.format_float_scientific(abs(x), unique=True, trim="-", exp_digits=1)     # d[.ddd]e[+-]x, shortest digits
    mant, exp = sci.split("e")
    digits = mant.replace(".", "")
    n, e10 = len(digits), int(exp)
    k = e10 - (n - 1)                                                                  # the exponent of the last digit
    kk = n + k                                                                         # where the decimal point stands
    if 0 <= k and kk <= 13:
        body = digits + "0" * k + ".0"
    elif 0 < kk <= 13:
        body = digits[:kk] + "." + digits[kk:]
    elif -6 < kk <= 0:
        body = "0." + "0" * (-kk) + digits
    elif n == 1:
        body = digits + "e%d" % (kk - 1)
    else:
        body = digits[0] + "." + digits[1:] + "e%d" % (kk - 1)
    return sign + body.encode()


def f32_text_of_bits(bits):
    return f32_text(f32_of_bits(bits))


def f32_texts(bits):
    """the texts of an array of bit patterns; equal patterns are formatted once"""
    uniq, inv = np.unique(np.asarray(bits, dtype=np.uint32), return_inverse=True)
    vals = uniq.view(np.float32)
    texts = [f32_text(v) for v in vals]
    return [texts[i] for i in inv]


def csv_field(name):
    """QuoteStyle::Necessary with a tab delimiter"""
    if any(c in name for c in b'\t"\r\n'):
        return b'"' + name.replace(b'"', b'""') + b'"'
    return name


def u64_f32(v):
    """a u64 as an f32, to nearest even (numpy converts the uint64 exactly as C does)"""
    return np.uint64(v).astype(np.float32)


def floats(c):
    """(identity, similarity, inv_size) of a record's counters (a dict over COUNT_FIELDS), numpy.float32"""
    aligned = (c["match"] + c["mismatch"] + c["del_bp"] + c["inv_del_bp"]) & U64
    with np.errstate(divide="ignore", invalid="ignore"):
        identity = u64_f32(c["match"]) / u64_f32(aligned)
        similarity = u64_f32((c["match"] + c["mismatch"]) & U64) / u64_f32(aligned)
        if c["inv_ev"] != 0:
            query_align = (c["match"] + c["mismatch"] + c["ins_bp"] + c["inv_ins_bp"]) & U64
            inv_size = u64_f32((aligned + query_align) & U64) / u64_f32((c["inv_ev"] + 1) & U64)
        else:
            inv_size = np.float32(0)
    return aligned, identity, similarity, inv_size


def row(ref_name, ref_size, ref_start, query_name, query_size, query_start, c):
    """one row; c = the record's counters, a dict over COUNT_FIELDS (or an 11-tuple in that order)"""
    if not isinstance(c, dict):
        c = dict(zip(COUNT_FIELDS, (int(v) for v in c)))
    aligned, identity, similarity, inv_size = floats(c)
    cols = [csv_field(ref_name), b"%d" % ref_size, b"%d" % ref_start, csv_field(query_name), b"%d" % query_size, b"%d" % query_start,
            b"%d" % aligned, b"0", f32_text(identity), f32_text(similarity)]
    cols += [b"%d" % c[k] for k in ("match", "mismatch", "ins_ev", "del_ev", "ins_bp", "del_bp", "inv_ev")]
    cols.append(f32_text(inv_size))
    cols += [b"%d" % c[k] for k in ("inv_ins_ev", "inv_ins_bp", "inv_del_ev", "inv_del_bp")]
    return b"\t".join(cols) + b"\n"


# ---- natord 1.0.9 `compare` (case-sensitive) ---------------------------------------------------------------------------------------
def _digit_run(s, at):
    """the end of the run of digits of s that starts at `at`"""
    while at < len(s) and s[at].isdigit():
        at += 1
    return at


def natord_compare(a, b):
    """-1 / 0 / 1 as natord::compare orders two strs.  compare_iter: in front of every step white space is skipped on both sides;
    two digits open a run on each side — with a leading zero on either the runs compare from the left like fractions (the first
    difference decides, then the longer run is greater), otherwise like numbers (the longer run is greater, then the first
    difference); anything else compares by character"""
    i = j = 0
    while True:
        while i < len(a) and a[i].isspace():
            i += 1
        while j < len(b) and b[j].isspace():
            j += 1
        if i == len(a) or j == len(b):
            return (i < len(a)) - (j < len(b))
        if a[i].isdigit() and b[j].isdigit():
            ra, rb = a[i:_digit_run(a, i)], b[j:_digit_run(b, j)]
            i, j = i + len(ra), j + len(rb)
            if ra[0] == "0" or rb[0] == "0":
                m = min(len(ra), len(rb))
                if ra[:m] != rb[:m]:
                    return -1 if ra[:m] < rb[:m] else 1
                if len(ra) != len(rb):
                    return -1 if len(ra) < len(rb) else 1
            elif len(ra) != len(rb):
                return -1 if len(ra) < len(rb) else 1
            elif ra != rb:
                return -1 if ra < rb else 1
            continue
        if a[i] != b[j]:
            return -1 if a[i] < b[j] else 1
        i, j = i + 1, j + 1


def sort_rows(ref_names, rows):
    """the rows in the order stat.rs:104 leaves them: stably by natord of ref_name"""
    order = sorted(range(len(rows)), key=functools.cmp_to_key(lambda x, y: natord_compare(ref_names[x], ref_names[y])))
    return [rows[k] for k in order]


def table(records):
    """the whole output for records = [(ref_name, ref_size, ref_start, query_name, query_size, query_start, counts)] (names as
    bytes): the header and the sorted rows, or nothing without a record"""
    if not records:
        return b""
    rows = [row(*r) for r in records]
    return HEADER + b"".join(sort_rows([r[0].decode("utf-8", "replace") for r in records], rows))
