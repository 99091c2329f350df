"""K34's part of the C-ABI: the three entries stand in the header, in the binding and in the library, the ABI version stays 3,
wga_dotplot_ov_head has its size and field offsets, the argument errors of wga_dotplot_overview and wga_f64_text (on the emulator
build: no GPU needed) — the restatement the K34 tests compare with is itself checked against the binary's `__fmt_f64` hook, and the
power-of-five tables of wga_f64_text.h against scripts/make_f64_text_tables.py, entry by entry."""
import importlib.util
import os
import re
import subprocess

from wgatools_amd import _lib
from wgatools_amd import build
from wgatools_amd import engine
import dotplot_overview_cases as k34

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_declares_the_three_entries():
    text = open(os.path.join(ROOT, "include", "wga_hip.h")).read()
    assert re.search(r"#define WGA_ABI_VERSION 3\b", text)
    assert re.search(r"uint64_t wga_dotplot_overview_work_bytes\(uint64_t n\);", text)
    assert re.search(r"int wga_dotplot_overview\(wga_ctx\*, uint32_t n, const uint8_t\* d_names, uint64_t n_name_bytes,\s+"
                     r"const wga_dotplot_ov_head\* d_heads, const wga_cigar_counts\* d_counts, int no_identity,\s+"
                     r"void\* d_work, uint64_t\* d_row_off /\* n \+ 1, device \*/, uint64_t\* total_bytes, uint8_t\* d_out\);", text)
    assert re.search(r"int wga_f64_text\(wga_ctx\*, uint64_t n, const uint64_t\* d_bits, uint8_t\* d_text /\* 32 n bytes \*/, "
                     r"uint8_t\* d_len\);", text)
    assert "dotplot.rs:384-423" in text
    assert text.count("8 * (n + n / 1024 + 4)") == 2                             # the d_work formula, K33's and K34's
    k34h = open(os.path.join(ROOT, "wgatools_amd", "csrc", "wga_k34_dotplot_overview.h")).read()
    assert "dotplot.rs:384-423" in k34h and "160 KiB" in k34h


def test_layout_and_prototypes(tmp_path):
    """tests/abi_layout_dotplot_overview.c: _Static_assert on the ABI version, the size and field offsets of wga_dotplot_ov_head,
    and the three entries assigned to pointers of the documented types"""
    r = subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), "-c",
                        os.path.join(ROOT, "tests", "abi_layout_dotplot_overview.c"), "-o", str(tmp_path / "abi_layout_dotplot_overview.o")],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout


def test_binding_carries_the_three_entries():
    assert len(_lib.PROTOTYPES["wga_dotplot_overview_work_bytes"][1]) == 1
    assert len(_lib.PROTOTYPES["wga_dotplot_overview"][1]) == 11
    assert len(_lib.PROTOTYPES["wga_f64_text"][1]) == 5
    dt = engine.DOTPLOT_OV_HEAD_DTYPE
    assert dt.itemsize == 64 and engine.COUNTS_DTYPE.itemsize == 88 and engine.COUNTS_DTYPE.fields["match"][1] == 0
    assert [dt.fields[k][1] for k in ("ref_start", "ref_end", "q_first", "q_second", "align_size", "rname_off", "qname_off",
                                      "rname_len", "qname_len")] == [0, 8, 16, 24, 32, 40, 48, 56, 60]
    for name in ("dotplot_overview", "f64_text"):
        assert hasattr(engine.Engine, name), name


def test_library_exports_the_three_entries(emu):
    assert emu.lib.wga_abi_version() == 3
    assert emu.lib.wga_dotplot_overview_work_bytes(0) == 8 * 4
    assert emu.lib.wga_dotplot_overview is not None and emu.lib.wga_f64_text is not None


def test_argument_errors(emu):
    k34.check_abi_arguments(emu)


def test_restatement_prints_f64_as_the_host_does():
    """dotplot_overview_ref.f64_text (numpy's Dragon4 digits under ryu's layout) against format_f64 (std::to_chars) through the
    binary's hidden hook, for the whole pattern list of the K34 tests; and the layouts of the named values by hand"""
    k34.check_ref_layouts()
    cli = build.build_cli_emu()
    bits, want = k34.f64_patterns()
    got = []
    for lo in range(0, len(bits), 1 << 12):                                       # 4 Ki patterns per command line
        r = subprocess.run([cli, "__fmt_f64"] + ["%016x" % b for b in bits[lo:lo + (1 << 12)]], stdout=subprocess.PIPE)
        assert r.returncode == 0
        got += r.stdout.split(b"\n")[:-1]
    assert len(got) == len(want)
    bad = [(hex(int(b)), g, w) for b, g, w in zip(bits, got, want) if g != w]
    assert not bad, (len(bad), bad[:10])


def test_f64_text_tables_are_the_script_s():
    """every entry of kF64Pow5 and kF64Pow5Inv in wga_f64_text.h is what scripts/make_f64_text_tables.py computes from Python
    integers; a few of them once more by hand"""
    spec = importlib.util.spec_from_file_location("make_f64_text_tables", os.path.join(ROOT, "scripts", "make_f64_text_tables.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    pow5, pow5_inv = gen.parse(open(gen.HEADER).read())
    want5, want5_inv = gen.tables()
    assert len(pow5) == 326 and len(pow5_inv) == 292
    assert pow5 == want5 and pow5_inv == want5_inv
    join = lambda r: r[0] | r[1] << 64
    for i in (0, 1, 27, 55, 56, 200, 325):
        p = 5 ** i
        b = p.bit_length()
        assert b == ((i * 1217359) >> 19) + 1                                     # f64_pow5_bits
        assert join(pow5[i]) == (p >> (b - 125) if b >= 125 else p << (125 - b)) and join(pow5[i]).bit_length() == 125
    for q in (0, 1, 21, 22, 290, 291):
        p = 5 ** q
        assert join(pow5_inv[q]) == (1 << (p.bit_length() - 1 + 125)) // p + 1
    assert all(((i * 1217359) >> 19) + 1 == (5 ** i).bit_length() for i in range(326))
    assert subprocess.run(["python3", os.path.join(ROOT, "scripts", "make_f64_text_tables.py")], stdout=subprocess.PIPE).returncode == 0
