"""K36's part of the C-ABI: the three entries stand in the header, in the binding and in the library, the ABI version stays 3,
wga_stat_pair has its size and field offsets, the argument errors of wga_stat_pairs and wga_stat_pair_rows (on the emulator build:
no GPU needed) — and the restatement the K36 tests compare with is itself checked against the host's stat_tsv through the command."""
import os
import re
import subprocess

from wgatools_amd import _lib
from wgatools_amd import build
from wgatools_amd import engine
import stat_pairs_cases as k36
import stat_pairs_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_declares_the_three_entries():
    text = open(os.path.join(ROOT, "include", "wga_hip.h")).read()
    assert re.search(r"#define WGA_ABI_VERSION 3\b", text)
    assert re.search(r"uint64_t wga_stat_pairs_work_bytes\(uint64_t n\);", text)
    assert re.search(r"int wga_stat_pairs\(wga_ctx\*, uint32_t n, const uint8_t\* d_names, uint64_t n_name_bytes, "
                     r"const wga_stat_row_head\* d_heads,\s+const wga_cigar_counts\* d_counts, void\* d_work, uint64_t\* n_pairs,\s+"
                     r"uint32_t\* d_pair_of_rec, const uint32_t\* d_inv_in, wga_stat_pair\* d_pairs, uint64_t cap_pairs\);", text)
    assert re.search(r"int wga_stat_pair_rows\(wga_ctx\*, uint32_t n, const uint8_t\* d_names, uint64_t n_name_bytes, "
                     r"const wga_stat_row_head\* d_heads,\s+const wga_cigar_counts\* d_sums, const uint32_t\* d_inv_bits, "
                     r"void\* d_work,\s+uint64_t\* d_row_off /\* n \+ 1, device \*/, uint64_t\* total_bytes, uint8_t\* d_out\);", text)
    assert "stat.rs:167-223" in text and "stat.rs:186-213" in text and "stat.rs:216" in text and "stat_pair_hash_bits" in text
    assert "4 * (6 * n + 2)" in text                                              # the d_work formula
    k36h = open(os.path.join(ROOT, "wgatools_amd", "csrc", "wga_k36_stat_pairs.h")).read()
    assert "stat.rs:167-223" in k36h and "wga_group.h" in k36h
    group = open(os.path.join(ROOT, "wgatools_amd", "csrc", "wga_group.h")).read()
    assert "hash(u32 i)" in group and "same(u32 i, u32 j)" in group


def test_layout_and_prototypes(tmp_path):
    """tests/abi_layout_stat_pairs.c: _Static_assert on the ABI version, the size and field offsets of wga_stat_pair, and the
    three entries assigned to pointers of the documented types"""
    r = subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), "-c",
                        os.path.join(ROOT, "tests", "abi_layout_stat_pairs.c"), "-o", str(tmp_path / "abi_layout_stat_pairs.o")],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout


def test_binding_carries_the_three_entries():
    assert len(_lib.PROTOTYPES["wga_stat_pairs_work_bytes"][1]) == 1
    assert len(_lib.PROTOTYPES["wga_stat_pairs"][1]) == 12
    assert len(_lib.PROTOTYPES["wga_stat_pair_rows"][1]) == 11
    dt = engine.STAT_PAIR_DTYPE
    assert dt.itemsize == 128 and engine.COUNTS_DTYPE.itemsize == 88
    assert [dt.fields[k][1] for k in ("first_rec", "n_recs", "ref_start", "query_start", "sum", "inv_size_bits", "pad")] == \
        [0, 8, 16, 24, 32, 120, 124]
    for name in ("stat_pairs", "stat_pair_rows"):
        assert hasattr(engine.Engine, name), name


def test_library_exports_the_three_entries(emu):
    assert emu.lib.wga_abi_version() == 3
    assert emu.lib.wga_stat_pairs_work_bytes(0) == 288
    assert emu.lib.wga_stat_pairs is not None and emu.lib.wga_stat_pair_rows is not None
    assert emu.get_param("stat_pair_hash_bits") == 64


def test_argument_errors(emu):
    k36.check_abi_arguments(emu)
    k36.check_rows_arguments(emu)


def test_restatement_is_the_hosts_table(tmp_path):
    """stat_pairs_ref.table against stat_tsv (WGA_STAT_WRITER=host) for a file whose pairs wrap around, repeat and carry inverted
    records: the two were written apart from each other"""
    cli = build.build_cli_emu()
    text, records = k36.paf_case(7, 150)
    paf = k36.write(tmp_path, "r.paf", text)
    rc, out, err = k36.run(cli, "stat", "-f", "paf", paf, env=k36.HOST_WRITER)
    assert (rc, err) == (0, "") and out == ref.table(records)
