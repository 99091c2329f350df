"""K26's part of the C-ABI: the two entries are declared in the header and carried by the binding, and the ABI version stays 3
(no GPU needed)."""
import os
import re

from wgatools_amd import _lib
from wgatools_amd import engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_declares_the_two_entries():
    text = open(os.path.join(ROOT, "include", "wga_hip.h")).read()
    assert re.search(r"uint64_t wga_dotplot_csv_work_bytes\(uint64_t n_rows\);", text)
    assert re.search(r"int wga_dotplot_csv\(wga_ctx\*, uint32_t n, const uint64_t\* d_segs, const uint64_t\* d_seg_off,", text)
    assert re.search(r"#define WGA_ABI_VERSION 3\b", text)


def test_binding_carries_the_two_entries():
    assert len(_lib.PROTOTYPES["wga_dotplot_csv_work_bytes"][1]) == 1
    assert len(_lib.PROTOTYPES["wga_dotplot_csv"][1]) == 9
    assert hasattr(engine.Engine, "dotplot_csv") and hasattr(engine.Engine, "dotplot_csv_count")
