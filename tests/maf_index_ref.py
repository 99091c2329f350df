"""A naive restatement of the BYTES `wgatools maf-index` writes (tools/index.rs:14-94 through serde_json::to_string): the index as
one line, the entries in order of first appearance, serde_json's escapes — and, for the C-ABI entry wga_maf_index (K35), of what
one piece of a file contributes.  Built over maf_ext_ref.blocks_with_offsets (the reader's rule for blocks and their offsets), not
over the code under test."""
import maf_ext_ref as mref

U64 = (1 << 64) - 1
_SHORT = {0x22: b'\\"', 0x5C: b"\\\\", 0x08: b"\\b", 0x0C: b"\\f", 0x0A: b"\\n", 0x0D: b"\\r", 0x09: b"\\t"}


def json_string(name):
    """serde_json's string: the quote, the backslash and the five short escapes, \\u00xx (lower case) for every other byte below
    0x20, everything else as it is"""
    out = bytearray(b'"')
    for ch in name:
        if ch in _SHORT:
            out += _SHORT[ch]
        elif ch < 0x20:
            out += b"\\u%04x" % ch
        else:
            out.append(ch)
    return bytes(out + b'"')


def interval(start, asize, strand, offset):
    """end = start + align_size mod 2^64 (a release build's sum)"""
    return b'{"start":%d,"end":%d,"strand":"%s","offset":%d}' % (start, (start + asize) & U64, strand, offset)


def _walk(blocks):
    """index.rs:30-68 over [(offset, rows)]: (entries in order of first appearance as [name, size, isref, [interval texts]], error)"""
    entries, at = [], {}
    for offset, rows in blocks:
        seen = []
        for ord_, (name, start, asize, strand, size, _seq) in enumerate(rows):
            if name in seen:
                return None, "Duplicate name `%s` in a record not allowed, please check or use `rename`" % name.decode("utf-8", "replace")
            seen.append(name)
            if name not in at:
                at[name] = len(entries)
                entries.append([name, size, ord_ == 0, []])
            elif entries[at[name]][2] != (ord_ == 0):
                return None, "Same sequence cannot be both reference and query!"
            entries[at[name]][3].append(interval(start, asize, strand, offset))
    return entries, None


def index_text(data):
    """(the index file's bytes, None) or (None, the error's message)"""
    entries, err = _walk(mref.blocks_with_offsets(data))
    if err:
        return None, err
    if not entries:
        return None, "Empty record"
    return b"{" + b",".join(b'%s:{"ivls":[%s],"size":%d,"isref":%s}' % (json_string(n), b",".join(iv), size, b"true" if isref else b"false")
                            for n, size, isref, iv in entries) + b"}", None


def piece_index(piece, skip=0, base=0, carry=0):
    """what wga_maf_index says about one piece: `piece` starts with the file's header line (skip = 0) or with the dummy line "#\\n"
    (skip = 2); base = the file position of piece[skip]; carry = the position behind the last record-ending line in front of the
    piece.  A dict: groups = [(name, size, isref, first_line, [interval texts])] by ascending first s-line, n_blocks, n_slines,
    first_dup_line, first_conflict_line (line indices or None) and next_offset."""
    assert skip in (0, 2) and (skip == 0 or piece[:2] == b"#\n")
    blocks = []
    for k, (off, rows) in enumerate(mref.blocks_with_offsets(piece)):
        # blocks_with_offsets starts behind the piece's first line: the header's end, or — behind the dummy line — where the carry stands in
        blocks.append((carry if skip and off == 2 else base + off - skip, rows))
    # the s-lines' line indices, in file order: the rows of the blocks in order
    lines = piece.split(b"\n")
    if lines and lines[-1] == b"":
        lines.pop()
    s_idx = [i for i, ln in enumerate(lines) if i > 0 and ln[:1] == b"s"]
    groups, at, dup, conflict, k = [], {}, None, None, 0
    for off, rows in blocks:
        seen = []
        for ord_, (name, start, asize, strand, size, _seq) in enumerate(rows):
            line = s_idx[k]
            k += 1
            if name in seen and dup is None:
                dup = line
            seen.append(name)
            if name not in at:
                at[name] = len(groups)
                groups.append([name, size, ord_ == 0, line, []])
            elif groups[at[name]][2] != (ord_ == 0) and conflict is None:
                conflict = line
            groups[at[name]][4].append(interval(start, asize, strand, off))
    assert k == len(s_idx)
    # the carry for the next piece: behind the last line that ended a run (the header line of a first piece stands in for one)
    pos, cur, in_run = 0, carry, False
    for i, ln in enumerate(lines):
        end = min(pos + len(ln) + 1, len(piece))
        if i == 0:
            if skip == 0:
                cur = base + end
        elif ln[:1] == b"s":
            in_run = True
        elif in_run:
            in_run, cur = False, base + end - skip
        pos = end
    return dict(groups=[tuple(g) for g in groups], n_blocks=len(blocks), n_slines=len(s_idx), first_dup_line=dup,
                first_conflict_line=conflict, next_offset=cur)
