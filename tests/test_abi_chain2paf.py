"""K27's part of the C-ABI: the two entries stand in the header, in the binding and in the library, the ABI version stays 3, and
the argument errors of wga_chain2paf (on the emulator build: no GPU needed)."""
import os
import re

from wgatools_amd import _lib
from wgatools_amd import engine
import chain2paf_cases as c2p

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_declares_the_two_entries():
    text = open(os.path.join(ROOT, "include", "wga_hip.h")).read()
    assert re.search(r"#define WGA_ABI_VERSION 3\b", text)
    assert re.search(r"uint64_t wga_chain2paf_work_bytes\(uint64_t n_chains, uint64_t n_data_lines\);", text)
    assert re.search(r"int wga_chain2paf\(wga_ctx\*, const uint8_t\* d_text, uint64_t n_bytes, const wga_chain_head\* d_heads, "
                     r"uint64_t n_chains,\s+const uint64_t\* d_lines, const uint64_t\* d_line_off, void\* d_work, "
                     r"uint64_t\* total_bytes, uint8_t\* d_out\);", text)


def test_binding_carries_the_two_entries():
    assert len(_lib.PROTOTYPES["wga_chain2paf_work_bytes"][1]) == 2
    assert len(_lib.PROTOTYPES["wga_chain2paf"][1]) == 10
    assert hasattr(engine.Engine, "chain2paf") and hasattr(engine.Engine, "chain2paf_count")


def test_library_exports_the_two_entries(emu):
    assert emu.lib.wga_abi_version() == 3
    assert emu.lib.wga_chain2paf_work_bytes(0, 0) >= 8
    assert emu.lib.wga_chain2paf is not None


def test_argument_errors(emu):
    c2p.check_abi_arguments(emu)
