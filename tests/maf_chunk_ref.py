"""An independent restatement of `wgatools chunk` (tools/chunk.rs:20-90, recount_align_size parser/common.rs:179-190, the
record writer maf.rs:566-581) over the MAF block reader's rules (maf.rs:25-36,138-211,371-421): the tests' expectation.

Reader: the first line is the header; a block is a maximal run of lines that start with `s`; every other line ends the block
in progress and is dropped; an s-line is seven white-space separated fields.  The `a` score is never parsed (score=255)."""


def read_blocks(text):
    """(blocks, error): blocks = [[(name, start, size, strand, src_size, seq), ...], ...] in input order; error = None, or
    the index of the block that holds the first s-line that does not parse (the blocks in front of it are returned)"""
    lines = text.split(b"\n")
    if lines and lines[-1] == b"":
        lines.pop()
    blocks, cur = [], None
    for i, ln in enumerate(lines):
        if ln.endswith(b"\r"):
            ln = ln[:-1]
        if i == 0:
            continue
        if ln[:1] != b"s":
            if cur is not None:
                blocks.append(cur)
            cur = None
            continue
        f = ln.split()
        ok = len(f) == 7 and f[2].isdigit() and f[3].isdigit() and f[5].isdigit() and f[4] in (b"+", b"-")
        if not ok:
            return blocks, len(blocks)
        if cur is None:
            cur = []
        cur.append((f[1], int(f[2]), int(f[3]), f[4], int(f[5]), f[6]))
    if cur is not None:
        blocks.append(cur)
    return blocks, None


def chunk_bounds(block_length, L):
    """chunk.rs:43-56: [0, L), [L, 2L), ... while the chunk ends before the block does, then [start, block_length)"""
    out, s, e = [], 0, L
    while e < block_length:
        out.append((s, e))
        s, e = e, e + L
    out.append((s, block_length))
    return out


def chunk_text(blocks, L):
    """(text, panic): the records of every block, up to the first chunk that slices a row shorter than its end (panic =
    (block, chunk) then, None otherwise).  The output header is not included."""
    out = []
    for b, rows in enumerate(blocks):
        ends = [r[1] for r in rows]
        for k, (c0, c1) in enumerate(chunk_bounds(len(rows[0][5]), L)):
            if any(len(r[5]) < c1 for r in rows):
                return b"".join(out), (b, k)
            rec = [b"a score=255\n"]
            for i, (name, _start, _size, strand, src, seq) in enumerate(rows):
                piece = seq[c0:c1]
                size = len(piece) - piece.count(b"-")
                rec.append(b"s\t%s\t%d\t%d\t%s\t%d\t%s\n" % (name, ends[i], size, strand, src, piece))
                ends[i] += size
            rec.append(b"\n")
            out.append(b"".join(rec))
    return b"".join(out), None


def header(L):
    return b"#maf version=1.6 split_length=%d\n" % L
