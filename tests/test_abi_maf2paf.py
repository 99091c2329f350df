"""K28's part of the C-ABI: the two entries and the head struct stand in the header, in the binding and in the library, the ABI
version stays 3, and the argument errors of wga_maf2paf (on the emulator build: no GPU needed)."""
import os
import re
import subprocess

from wgatools_amd import _lib
from wgatools_amd import engine
import maf2paf_cases as m2p

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_declares_the_two_entries_and_the_struct():
    text = open(os.path.join(ROOT, "include", "wga_hip.h")).read()
    assert re.search(r"#define WGA_ABI_VERSION 3\b", text)
    assert re.search(r"\} wga_maf2paf_head;", text)
    assert re.search(r"uint64_t wga_maf2paf_work_bytes\(uint64_t n, uint64_t n_runs\);", text)
    assert re.search(r"int wga_maf2paf\(wga_ctx\*, uint32_t n, const uint8_t\* d_names, uint64_t n_name_bytes, "
                     r"const wga_maf2paf_head\* d_heads,\s+const wga_cigar_counts\* d_counts, const uint64_t\* d_runs, "
                     r"const uint64_t\* d_run_off, const uint64_t\* d_cols,\s+void\* d_work, uint64_t\* total_bytes, "
                     r"uint8_t\* d_out\);", text)
    assert "maf.rs:484-520" in text and "converter.rs:29-54" in text


def test_struct_layout(tmp_path):
    """tests/abi_layout_maf2paf.c: _Static_assert on the size of and every offset in wga_maf2paf_head, and on the ABI version"""
    r = subprocess.run(["gcc", "-std=c11", "-I" + os.path.join(ROOT, "include"), "-c", os.path.join(ROOT, "tests", "abi_layout_maf2paf.c"),
                        "-o", str(tmp_path / "abi_layout_maf2paf.o")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout


def test_head_dtype_matches_the_header():
    dt = engine.MAF2PAF_HEAD_DTYPE
    assert dt.itemsize == 80
    assert {k: dt.fields[k][1] for k in dt.names} == {
        "q": 0, "t": 24, "qname_off": 48, "tname_off": 56, "qname_len": 64, "tname_len": 68, "strand_neg": 72, "pad": 73}


def test_binding_carries_the_two_entries():
    assert len(_lib.PROTOTYPES["wga_maf2paf_work_bytes"][1]) == 2
    assert len(_lib.PROTOTYPES["wga_maf2paf"][1]) == 12
    assert hasattr(engine.Engine, "maf2paf") and hasattr(engine.Engine, "maf2paf_count")


def test_library_exports_the_two_entries(emu):
    assert emu.lib.wga_abi_version() == 3
    assert emu.lib.wga_maf2paf_work_bytes(0, 0) >= 8
    assert emu.lib.wga_maf2paf is not None


def test_argument_errors(emu):
    m2p.check_abi_arguments(emu)
