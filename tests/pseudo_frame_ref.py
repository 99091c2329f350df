"""K31's contract (include/wga_hip.h, wga_pafpseudo_frame) restated with numpy: the items applied one after the other up to
the first bad one."""
import numpy as np

FILL, COPY_POOL, COPY_TEXT, HOLE = 0, 1, 2, 3
NONE = 0xFFFFFFFFFFFFFFFF
M64 = (1 << 64) - 1


def first_bad(items, pool_bytes, text_bytes, out_bytes):
    """the index of the first item that breaks the tiling, has an unknown kind or copies from outside its source, or None"""
    end = 0
    for k, (dst, ln, src, kind) in enumerate(items):
        if dst != end or ln > out_bytes or dst > out_bytes - ln or kind > HOLE:
            return k
        if kind == COPY_POOL and (ln > pool_bytes or src > pool_bytes - ln):
            return k
        if kind == COPY_TEXT and (ln > text_bytes or src > text_bytes - ln):
            return k
        end = (dst + ln) & M64
        if k + 1 == len(items) and end != out_bytes:
            return k
    return None


def apply(items, pool, text, before):
    """`before` = the buffer's out_bytes bytes before the call (numpy u8); returns (the bytes after it, first bad item or None)"""
    out = np.array(before, dtype=np.uint8, copy=True)
    bad = first_bad(items, len(pool), len(text), len(out))
    for k, (dst, ln, src, kind) in enumerate(items):
        if k == bad:
            break
        if kind == FILL:
            out[dst:dst + ln] = src & 0xFF
        elif kind == COPY_POOL:
            out[dst:dst + ln] = pool[src:src + ln]
        elif kind == COPY_TEXT:
            out[dst:dst + ln] = text[src:src + ln]
    return out, bad
