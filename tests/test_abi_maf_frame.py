"""K32's part of the C-ABI: the two entries stand in the header, in the binding and in the library, the ABI version stays 3,
wga_maf_frame_head has its 88 bytes and field offsets, and the argument errors of wga_paf2maf_frame (on the emulator build: no
GPU needed)."""
import os
import re
import subprocess

from wgatools_amd import _lib
from wgatools_amd import engine
import maf_frame_cases as k32

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_declares_the_two_entries():
    text = open(os.path.join(ROOT, "include", "wga_hip.h")).read()
    assert re.search(r"#define WGA_ABI_VERSION 3\b", text)
    assert re.search(r"uint64_t wga_paf2maf_frame_work_bytes\(uint64_t n\);", text)
    assert re.search(r"int wga_paf2maf_frame\(wga_ctx\*, uint32_t n, const uint8_t\* d_names, uint64_t n_name_bytes,\s+"
                     r"const wga_maf_frame_head\* d_heads, const wga_cigar_counts\* d_counts,\s+"
                     r"const uint64_t\* d_t_src_len, const uint64_t\* d_q_src_len,\s+"
                     r"const wga_rec_diag\* d_diag, void\* d_work,\s+"
                     r"uint64_t\* d_t_row_off, uint64_t\* d_q_row_off, uint64_t\* d_rec_off,\s+"
                     r"uint64_t\* total_bytes, uint32_t\* n_good, uint64_t\* good_bytes, uint8_t\* d_out\);", text)
    assert "maf.rs:566-581" in text and "converter.rs:196-263" in text and ":288-355" in text
    assert "8 * (2 n + 2 + n / 1024 + 4)" in text                                 # the d_work formula


def test_layout_and_prototypes(tmp_path):
    """tests/abi_layout_maf_frame.c: _Static_assert on the ABI version, the size and field offsets of wga_maf_frame_head and the
    sizes of the structs K32 reads, and the two entries assigned to pointers of the documented types"""
    r = subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), "-c",
                        os.path.join(ROOT, "tests", "abi_layout_maf_frame.c"), "-o", str(tmp_path / "abi_layout_maf_frame.o")],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout


def test_binding_carries_the_two_entries():
    assert len(_lib.PROTOTYPES["wga_paf2maf_frame_work_bytes"][1]) == 1
    assert len(_lib.PROTOTYPES["wga_paf2maf_frame"][1]) == 17
    dt = engine.MAF_FRAME_HEAD_DTYPE
    assert dt.itemsize == 88 and engine.COUNTS_DTYPE.itemsize == 88 and engine.DIAG_DTYPE.itemsize == 24
    assert [dt.fields[k][1] for k in ("score", "t", "q", "tname_off", "qname_off", "tname_len", "qname_len", "t_neg", "q_neg")] == \
        [0, 8, 32, 56, 64, 72, 76, 80, 81]
    for name in ("maf_frame", "maf_frame_count", "maf_records", "download_slice"):
        assert hasattr(engine.Engine, name), name


def test_library_exports_the_two_entries(emu):
    assert emu.lib.wga_abi_version() == 3
    assert emu.lib.wga_paf2maf_frame_work_bytes(0) == 8 * (2 + 4)
    assert emu.lib.wga_paf2maf_frame is not None


def test_argument_errors(emu):
    k32.check_abi_arguments(emu)
