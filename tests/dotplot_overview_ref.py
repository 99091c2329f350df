"""What `dotplot -m overview --out-format csv` prints, restated from the reference (rec_dot_data tools/dotplot.rs:384-423 through the
csv writer of render_output) — independently of the kernel and of the host's dotplot_rows:
  * identity is numpy.float64 division of np.uint64(...).astype(np.float64) (conversion to nearest even, IEEE division);
  * its digits are numpy's Dragon4 in unique mode (format_float_scientific), laid out by ryu's rules (pretty::format64);
  * csv quoting (QuoteStyle::Necessary, comma delimiter) is restated here.
test_abi_dotplot_overview.py checks f64_text against the binary's hidden `__fmt_f64` hook (std::to_chars) for the whole pattern
list."""
import numpy as np

U64 = (1 << 64) - 1
HEADER = b"ref_start,ref_end,query_start,query_end,identity,ref_chro,query_chro\n"


def f64_of_bits(bits):
    return np.array([bits], dtype=np.uint64).view(np.float64)[0]


def f64_text(x):
    """ryu::Buffer::format(f64): x a numpy.float64"""
    x = np.float64(x)
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
    if 0 <= k and kk <= 16:
        body = digits + "0" * k + ".0"
    elif 0 < kk <= 16:
        body = digits[:kk] + "." + digits[kk:]
    elif -5 < kk <= 0:
        body = "0." + "0" * (-kk) + digits
    elif n == 1:
        body = digits + "e%d" % (kk - 1)
    else:
        body = digits[0] + "." + digits[1:] + "e%d" % (kk - 1)
    return sign + body.encode()


def f64_text_of_bits(bits):
    return f64_text(f64_of_bits(bits))


def f64_texts(bits):
    """the texts of an array of bit patterns; equal patterns are formatted once"""
    uniq, inv = np.unique(np.asarray(bits, dtype=np.uint64), return_inverse=True)
    vals = uniq.view(np.float64)
    texts = [f64_text(v) for v in vals]
    return [texts[i] for i in inv]


def csv_field(name):
    """QuoteStyle::Necessary with a comma delimiter"""
    if any(c in name for c in b',"\r\n'):
        return b'"' + name.replace(b'"', b'""') + b'"'
    return name


def identity(match, align_size):
    """(double)match / (double)align_size, numpy.float64 (numpy converts the uint64 exactly as C does)"""
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.uint64(match).astype(np.float64) / np.uint64(align_size).astype(np.float64)


def row(ref_start, ref_end, q_first, q_second, ref_name, query_name, match=0, align_size=0, no_identity=False):
    """one row; the four numbers as printed (the query pair of a `-` record swapped already)"""
    ident = b"1.0" if no_identity else f64_text(identity(match, align_size))
    return b",".join([b"%d" % ref_start, b"%d" % ref_end, b"%d" % q_first, b"%d" % q_second, ident, csv_field(ref_name),
                      csv_field(query_name)]) + b"\n"


def record_row(ref_name, ref_start, ref_end, query_name, query_start, query_end, neg, match, no_identity=False):
    """the row of a record (dotplot.rs:400-406: a `-` record prints its query end first); the divisor is the target span"""
    qa, qb = (query_end, query_start) if neg else (query_start, query_end)
    return row(ref_start, ref_end, qa, qb, ref_name, query_name, match, ref_end - ref_start, no_identity)


def table(records, no_identity=False):
    """the whole output for records = [(ref_name, ref_start, ref_end, query_name, query_start, query_end, neg, match)]: the
    header and the rows in input order, or nothing without a record"""
    if not records:
        return b""
    return HEADER + b"".join(record_row(*r, no_identity=no_identity) for r in records)
