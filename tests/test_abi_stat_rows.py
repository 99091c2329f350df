"""K33's part of the C-ABI: the three entries stand in the header, in the binding and in the library, the ABI version stays 3,
wga_stat_row_head has its size and field offsets, the argument errors of wga_stat_rows and wga_f32_text (on the emulator build: no
GPU needed) — and the restatement the K33 tests compare with is itself checked against the binary's `__fmt_f32` and `__natord`
hooks.

The struct: four 64-bit numbers, two 64-bit offsets and two 32-bit lengths are 56 bytes (the issue that asked for K33 spelled the
fields out and counted 48; the fields are what a caller fills, so they stand and the size follows from them)."""
import os
import re
import subprocess

from wgatools_amd import _lib
from wgatools_amd import build
from wgatools_amd import engine
import stat_rows_cases as k33
import stat_rows_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_declares_the_three_entries():
    text = open(os.path.join(ROOT, "include", "wga_hip.h")).read()
    assert re.search(r"#define WGA_ABI_VERSION 3\b", text)
    assert re.search(r"uint64_t wga_stat_rows_work_bytes\(uint64_t n\);", text)
    assert re.search(r"int wga_stat_rows\(wga_ctx\*, uint32_t n, const uint8_t\* d_names, uint64_t n_name_bytes,\s+"
                     r"const wga_stat_row_head\* d_heads, const wga_cigar_counts\* d_counts,\s+"
                     r"void\* d_work, uint64_t\* d_row_off /\* n \+ 1, device \*/, uint64_t\* total_bytes, uint8_t\* d_out\);", text)
    assert re.search(r"int wga_f32_text\(wga_ctx\*, uint64_t n, const uint32_t\* d_bits, uint8_t\* d_text, uint8_t\* d_len\);", text)
    assert "stat.rs:129-164" in text and "stat.rs:117-123" in text and "common.rs:116-140" in text
    assert "8 * (n + n / 1024 + 4)" in text                                       # the d_work formula
    k33h = open(os.path.join(ROOT, "wgatools_amd", "csrc", "wga_k33_stat_rows.h")).read()
    assert "stat.rs:129-164" in k33h and "stat.rs:117-123" in k33h and "common.rs:116-140" in k33h


def test_layout_and_prototypes(tmp_path):
    """tests/abi_layout_stat_rows.c: _Static_assert on the ABI version, the size and field offsets of wga_stat_row_head, and the
    three entries assigned to pointers of the documented types"""
    r = subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), "-c",
                        os.path.join(ROOT, "tests", "abi_layout_stat_rows.c"), "-o", str(tmp_path / "abi_layout_stat_rows.o")],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout


def test_binding_carries_the_three_entries():
    assert len(_lib.PROTOTYPES["wga_stat_rows_work_bytes"][1]) == 1
    assert len(_lib.PROTOTYPES["wga_stat_rows"][1]) == 10
    assert len(_lib.PROTOTYPES["wga_f32_text"][1]) == 5
    dt = engine.STAT_ROW_HEAD_DTYPE
    assert dt.itemsize == 56 and engine.COUNTS_DTYPE.itemsize == 88
    assert [dt.fields[k][1] for k in ("ref_size", "ref_start", "query_size", "query_start", "rname_off", "qname_off", "rname_len",
                                      "qname_len")] == [0, 8, 16, 24, 32, 40, 48, 52]
    for name in ("stat_rows", "stat_rows_count", "f32_text"):
        assert hasattr(engine.Engine, name), name


def test_library_exports_the_three_entries(emu):
    assert emu.lib.wga_abi_version() == 3
    assert emu.lib.wga_stat_rows_work_bytes(0) == 8 * 4
    assert emu.lib.wga_stat_rows is not None and emu.lib.wga_f32_text is not None


def test_argument_errors(emu):
    k33.check_abi_arguments(emu)


def test_restatement_prints_f32_as_the_host_does():
    """stat_rows_ref.f32_text (numpy's Dragon4 digits under ryu's layout) against format_f32 (std::to_chars) through the binary's
    hidden hook, for the whole pattern list of the K33 tests; and the layouts of the named values by hand"""
    k33.check_ref_layouts()
    cli = build.build_cli_emu()
    bits, want = k33.f32_patterns()
    got = []
    for lo in range(0, len(bits), 1 << 14):                                       # 16 Ki patterns per command line
        r = subprocess.run([cli, "__fmt_f32"] + ["%08x" % b for b in bits[lo:lo + (1 << 14)]], stdout=subprocess.PIPE)
        assert r.returncode == 0
        got += r.stdout.split(b"\n")[:-1]
    assert len(got) == len(want)
    bad = [(hex(int(b)), g, w) for b, g, w in zip(bits, got, want) if g != w]
    assert not bad, (len(bad), bad[:10])


def test_restatement_orders_names_as_the_host_does():
    cli = build.build_cli_emu()
    names = ["c 1", "c1", "c10", "c2", "c01", "c001", "c 10", "chr1", "chr 1a", "1 2", "12", "a", "", "a 0", "a00", "x9", "x10", "x 9 ",
             "ref.chr8", "ref.chr10", "ref.chr 8"]
    pairs = [(a, b) for a in names for b in names]
    r = subprocess.run([cli, "__natord"] + [x for p in pairs for x in p], stdout=subprocess.PIPE, text=True)
    assert [int(v) for v in r.stdout.split()] == [ref.natord_compare(a, b) for a, b in pairs]
    assert ref.natord_compare("c 1", "c1") == 0 and ref.natord_compare("c2", "c10") < 0 and ref.natord_compare("c1", "c2") < 0
