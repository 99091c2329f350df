"""K30's part of the C-ABI: the two entries stand in the header, in the binding and in the library, the ABI version stays 3 and
wga_maf2paf_head keeps its 80 bytes, and the argument errors of wga_chain_heads (on the emulator build: no GPU needed)."""
import os
import re
import subprocess

from wgatools_amd import _lib
from wgatools_amd import engine
import chain_heads_cases as k30

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_declares_the_two_entries():
    text = open(os.path.join(ROOT, "include", "wga_hip.h")).read()
    assert re.search(r"#define WGA_ABI_VERSION 3\b", text)
    assert re.search(r"uint64_t wga_chain_heads_work_bytes\(uint64_t n\);", text)
    assert re.search(r"int wga_chain_heads\(wga_ctx\*, uint32_t n, const uint8_t\* d_names, uint64_t n_name_bytes, "
                     r"const wga_maf2paf_head\* d_heads,\s+const wga_chain_trim_t\* d_trim, const uint64_t\* d_nbytes, "
                     r"const wga_rec_diag\* d_diag,\s+uint64_t chain_id0, void\* d_work, uint64_t\* d_data_off, "
                     r"uint64_t\* total_bytes, uint32_t\* n_good,\s+uint8_t\* d_out\);", text)
    assert "chain.rs:185-203" in text and "chain.rs:103-183" in text
    assert "8 * (2 n + 2 + n / 1024 + 4)" in text                                 # the d_work formula


def test_layout_and_prototypes(tmp_path):
    """tests/abi_layout_chain_heads.c: _Static_assert on the ABI version and the sizes of the structs K30 reads, and the two
    entries assigned to pointers of the documented types"""
    r = subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), "-c",
                        os.path.join(ROOT, "tests", "abi_layout_chain_heads.c"), "-o", str(tmp_path / "abi_layout_chain_heads.o")],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout


def test_binding_carries_the_two_entries():
    assert len(_lib.PROTOTYPES["wga_chain_heads_work_bytes"][1]) == 1
    assert len(_lib.PROTOTYPES["wga_chain_heads"][1]) == 14
    assert engine.MAF2PAF_HEAD_DTYPE.itemsize == 80 and engine.CHAIN_TRIM_DTYPE.itemsize == 32 and engine.DIAG_DTYPE.itemsize == 24
    for name in ("chain_heads", "chain_heads_count", "chain_records"):
        assert hasattr(engine.Engine, name), name


def test_library_exports_the_two_entries(emu):
    assert emu.lib.wga_abi_version() == 3
    assert emu.lib.wga_chain_heads_work_bytes(0) >= 8
    assert emu.lib.wga_chain_heads is not None


def test_argument_errors(emu):
    k30.check_abi_arguments(emu)
