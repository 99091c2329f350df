"""Raw DEFLATE (RFC 1951) streams built by hand, for the tests of the device inflate (K17).

An encoder emits a small part of the legal streams and almost none of the illegal ones; this module writes any of them:
every header field, code length, repeat symbol and length / distance symbol is the caller's choice.  zlib is the judge of
what a stream means (zlib_verdict).

    bits = Bits()
    stored(bits, b"abc", final=False)
    fixed(bits, [65, ("match", 3, 1), "eob"], final=True)
    payload = bits.bytes()
"""
import zlib

CL_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)
LEN_BASE = (3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258)
LEN_EXTRA = (0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0)
DIST_BASE = (1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097,
             6145, 8193, 12289, 16385, 24577)
DIST_EXTRA = (0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13)
FIXED_LITLEN = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_DIST = [5] * 32          # 30 and 31 have codes, and no meaning (3.2.6)


class Bits:
    """the bit stream of 3.1.1: bytes fill from their least significant bit; header fields and extra bits go in least
    significant bit first, Huffman codes most significant bit first"""

    def __init__(self):
        self.acc = 0
        self.n = 0

    def field(self, value, nbits):
        assert 0 <= value < (1 << nbits) or nbits == 0 and value == 0, (value, nbits)
        self.acc |= value << self.n
        self.n += nbits

    def code(self, code, nbits):
        for k in range(nbits - 1, -1, -1):
            self.field((code >> k) & 1, 1)

    def align(self):
        self.n = (self.n + 7) & ~7

    def raw(self, data):
        assert self.n % 8 == 0
        self.acc |= int.from_bytes(data, "little") << self.n
        self.n += 8 * len(data)

    def bytes(self):
        return self.acc.to_bytes((self.n + 7) // 8, "little")


def canonical(lengths):
    """symbol -> (code, length) of the canonical code of 3.2.2; lengths need not be complete (an over-subscribed set gives
    codes that do not fit their length: such a set is only good for a header no symbol follows)"""
    count = [0] * 16
    for l in lengths:
        count[l] += 1
    count[0] = 0
    nxt, code = [0] * 16, 0
    for l in range(1, 16):
        code = (code + count[l - 1]) << 1
        nxt[l] = code
    out = {}
    for s, l in enumerate(lengths):
        if l:
            out[s] = (nxt[l], l)
            nxt[l] += 1
    return out


def length_symbol(n):
    """(symbol, extra bits, value) the way every encoder writes a match length: 258 is symbol 285"""
    assert 3 <= n <= 258
    if n == 258:
        return 285, 0, 0
    k = max(i for i in range(28) if LEN_BASE[i] <= n)
    return 257 + k, LEN_EXTRA[k], n - LEN_BASE[k]


def dist_symbol(d):
    assert 1 <= d <= 32768
    k = max(i for i in range(30) if DIST_BASE[i] <= d)
    return k, DIST_EXTRA[k], d - DIST_BASE[k]


def put_symbols(bits, symbols, litlen, dist):
    """symbols: literals (0..255), "eob", ("match", len, dist[, length symbol]) — the length symbol forced, e.g. 284 with
    extra bits 31 for 258 —, and for streams that break the format ("lit", s): the literal/length symbol s as it is
    (286, 287), ("rawmatch", length symbol, extra value, distance symbol, extra value)"""
    for s in symbols:
        if s == "eob":
            bits.code(*litlen[256])
        elif isinstance(s, int):
            bits.code(*litlen[s])
        elif s[0] == "lit":
            bits.code(*litlen[s[1]])
        elif s[0] == "match":
            ls, le, lv = length_symbol(s[1])
            if len(s) > 3:
                ls = s[3]
                le, lv = LEN_EXTRA[ls - 257], s[1] - LEN_BASE[ls - 257]
            bits.code(*litlen[ls])
            bits.field(lv, le)
            ds, de, dv = dist_symbol(s[2])
            bits.code(*dist[ds])
            bits.field(dv, de)
        elif s[0] == "rawmatch":
            _, ls, lv, ds, dv = s
            bits.code(*litlen[ls])
            bits.field(lv, LEN_EXTRA[ls - 257] if ls - 257 < 29 else 0)
            bits.code(*dist[ds])
            bits.field(dv, DIST_EXTRA[ds] if ds < 30 else 0)
        else:
            raise ValueError(s)


def stored(bits, data, final, nlen=None, length=None):
    """3.2.4; nlen / length: the header's NLEN and LEN as they are (default: the data's)"""
    bits.field(1 if final else 0, 1)
    bits.field(0, 2)
    bits.align()
    n = len(data) if length is None else length
    bits.field(n, 16)
    bits.field((~n & 0xFFFF) if nlen is None else nlen, 16)
    bits.raw(bytes(data))


def fixed(bits, symbols, final):
    """3.2.6"""
    bits.field(1 if final else 0, 1)
    bits.field(1, 2)
    put_symbols(bits, symbols, canonical(FIXED_LITLEN), canonical(FIXED_DIST))


def block_type(bits, btype, final):
    """a block header and nothing else (type 3)"""
    bits.field(1 if final else 0, 1)
    bits.field(btype, 2)


def cl_plain(lengths):
    """every code length spelled out: no 16 / 17 / 18"""
    return [(l,) for l in lengths]


def cl_rle(lengths):
    """the greedy run-length form an encoder would choose"""
    out, i, n = [], 0, len(lengths)
    while i < n:
        l, j = lengths[i], i
        while j < n and lengths[j] == l:
            j += 1
        run = j - i
        if l == 0:
            while run >= 11:
                r = min(run, 138)
                out.append((18, r))
                run -= r
            if run >= 3:
                out.append((17, run))
                run = 0
            out += [(0,)] * run
        else:
            out.append((l,))
            run -= 1
            while run >= 3:
                r = min(run, 6)
                out.append((16, r))
                run -= r
            out += [(l,)] * run
        i = j
    return out


def dynamic(bits, litlen_lengths, dist_lengths, symbols, final, cl_symbols=None, cl_lengths=None, hlit=None, hdist=None,
            hclen=None):
    """3.2.7.  litlen_lengths (257..286 of them; more for HLIT = 30 / 31) and dist_lengths (1..30; more for HDIST = 30 /
    31) give the canonical codes of the symbols.
    cl_symbols: the code-length alphabet's symbols as written, (length,), (16, repeat 3..6), (17, repeat 3..10) or (18,
    repeat 11..138), over the literal/length lengths and the distance lengths as one sequence — nothing checks that they
    spell the two sets (a 16 in front, a repeat past the end); default: cl_rle.
    cl_lengths: the 19 lengths of the code-length code by symbol; default: a complete code over the symbols in use.
    hlit / hdist / hclen: the raw header fields; default: from the sets, and the shortest HCLEN."""
    if cl_symbols is None:
        cl_symbols = cl_rle(list(litlen_lengths) + list(dist_lengths))
    if cl_lengths is None:
        used = sorted({s[0] for s in cl_symbols})
        if len(used) == 1:
            used.append(0 if used[0] else 1)     # a complete code needs two symbols
        k = max(1, (len(used) - 1).bit_length())
        short = (1 << k) - len(used)             # `short` codes of k - 1 bits, the others of k bits: Kraft sum 1
        cl_lengths = [0] * 19
        for i, s in enumerate(used):
            cl_lengths[s] = k - 1 if i < short else k
    if hclen is None:
        hclen = max([4] + [i + 1 for i in range(19) if cl_lengths[CL_ORDER[i]]]) - 4
    bits.field(1 if final else 0, 1)
    bits.field(2, 2)
    bits.field(len(litlen_lengths) - 257 if hlit is None else hlit, 5)
    bits.field(len(dist_lengths) - 1 if hdist is None else hdist, 5)
    bits.field(hclen, 4)
    for i in range(hclen + 4):
        bits.field(cl_lengths[CL_ORDER[i]], 3)
    cl = canonical(cl_lengths)
    for s in cl_symbols:
        bits.code(*cl[s[0]])
        if s[0] == 16:
            bits.field(s[1] - 3, 2)
        elif s[0] == 17:
            bits.field(s[1] - 3, 3)
        elif s[0] == 18:
            bits.field(s[1] - 11, 7)
    put_symbols(bits, symbols, canonical(litlen_lengths), canonical(dist_lengths))


def zlib_verdict(payload, out_len):
    """the bytes of the raw DEFLATE stream `payload` iff zlib raises nothing, reaches the end of the final block and made
    exactly out_len bytes (what lies behind the final block does not matter); else None"""
    d = zlib.decompressobj(-15)
    try:
        out = d.decompress(bytes(payload))
    except zlib.error:
        return None
    if not d.eof or len(out) != out_len:
        return None
    return out
