"""What a fill of an item stream (k_text_items_fill: K25, K26, K27) leaves alone when its total or its scan is not the count
call's.  Shared by chain_filter_cases.py, chain2paf_cases.py and dotplot_csv_cases.py: each builds a Stream of about 600 items
(three blocks of 256) behind its own count call and hands it to the two checks.  The output buffer always holds the true total
and a guard on both sides, so no write can leave the allocation."""
import numpy as np

ITEMS = 256      # items per block of the fill
GUARD = 64
CANARY = 0xA5    # no text holds it: all of them are ASCII


class Stream:
    """a counted stream.  work: the call's d_work with the scan of the item sizes at u64 word `scan_word` (the layout in the
    launcher's comment); want: the text; fill(total_bytes, d_out): the fill call with that *total_bytes"""

    def __init__(self, eng, work, scan_word, n_items, want, fill):
        self.eng, self.work, self.scan_word, self.n, self.want, self.fill = eng, work, scan_word, n_items, want, fill
        self.isc = [int(v) for v in work.numpy().view(np.uint64)[scan_word:scan_word + n_items + 1]]
        assert 2 * ITEMS < n_items <= 3 * ITEMS and self.isc[0] == 0 and self.isc[-1] == len(want) and CANARY not in want

    def filled(self, total):
        """the text's bytes after a fill into canaries; the guards are checked here"""
        out = self.eng.upload(np.full(len(self.want) + 2 * GUARD, CANARY, dtype=np.uint8))
        self.fill(total, out.ptr + GUARD)
        self.eng.sync()
        got = out.numpy()
        assert (got[:GUARD] == CANARY).all() and (got[GUARD + len(self.want):] == CANARY).all(), total
        return got[GUARD:GUARD + len(self.want)]


def check_short_total(st):
    """*total_bytes one below the true total, and the scan's value at item 256: a block that ends behind it writes nothing, the
    blocks wholly in front of it write their text"""
    for total, blocks_in_front in ((len(st.want) - 1, 2), (st.isc[ITEMS], 1)):
        got = st.filled(total)
        assert (got[total:] == CANARY).all(), total
        in_front = 0
        for x0 in range(0, st.n, ITEMS):
            e0, e1 = st.isc[x0], st.isc[min(x0 + ITEMS, st.n)]
            if e1 <= total:
                assert got[e0:e1].tobytes() == st.want[e0:e1], (total, x0)
                in_front += 1
        assert in_front == blocks_in_front, (total, in_front)


def check_scan_one_off(st, size_checked, k=ITEMS + ITEMS // 2):
    """scan entry k, in the middle of the second block, one lower: item k - 1 is one byte shorter and item k one byte longer than
    their texts.  Nothing outside the text changes (Stream.filled); a format whose fill checks the sizes (kCheckSize: K26)
    writes neither of the two and every other item"""
    lo, hi = st.isc[k - 1], st.isc[k + 1]
    assert lo < st.isc[k] < hi
    host = st.work.numpy()
    words = host.view(np.uint64)
    assert int(words[st.scan_word + k]) == st.isc[k]
    words[st.scan_word + k] -= 1
    st.eng.copy_into(st.work, host)
    got = st.filled(len(st.want))
    if not size_checked:
        return
    assert (got[lo:hi] == CANARY).all(), got[lo:hi].tobytes()
    assert got[:lo].tobytes() == st.want[:lo] and got[hi:].tobytes() == st.want[hi:]
