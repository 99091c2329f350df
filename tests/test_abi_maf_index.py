"""K35's part of the C-ABI: the two entries stand in the header, in the binding and in the library, the ABI version stays 3,
wga_maf_index_name has its size and field offsets, the argument errors of wga_maf_index (on the emulator build: no GPU needed), and
the restatement the K35 tests compare with agrees with the JSON module and with maf_ext_ref.build_index on the fixtures."""
import json
import os
import re
import subprocess

from wgatools_amd import _lib
from wgatools_amd import engine
from helpers import GOLDEN
import maf_ext_ref as mref
import maf_index_cases as k35
import maf_index_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_declares_the_two_entries():
    text = open(os.path.join(ROOT, "include", "wga_hip.h")).read()
    assert re.search(r"#define WGA_ABI_VERSION 3\b", text)
    assert re.search(r"WGA_E_FALLBACK = -6\b", text)
    assert re.search(r"uint64_t wga_maf_index_work_bytes\(uint64_t n_lines\);", text)
    assert re.search(r"int wga_maf_index\(wga_ctx\*, const uint8_t\* d_text, uint64_t n_bytes, const wga_maf_line\* d_lines, "
                     r"uint64_t n_lines, uint32_t skip,\s+uint64_t base, uint64_t carry_offset, void\* d_work, uint64_t\* n_names, "
                     r"uint64_t\* n_blocks, uint64_t\* n_slines,\s+uint64_t\* text_bytes, uint64_t\* first_dup_line, "
                     r"uint64_t\* first_conflict_line, uint64_t\* next_offset,\s+wga_maf_index_name\* d_names "
                     r"/\* \*n_names \+ 1, device \*/, uint8_t\* d_out\);", text)
    assert "index.rs:14-94" in text and "maf_index_hash_bits" in text and "maf_index_sort_bits" in text
    k35h = open(os.path.join(ROOT, "wgatools_amd", "csrc", "wga_k35_maf_index.h")).read()
    assert "index.rs:14-94" in k35h
    assert "stable" in open(os.path.join(ROOT, "wgatools_amd", "csrc", "wga_sort.h")).read()


def test_layout_and_prototypes(tmp_path):
    """tests/abi_layout_maf_index.c: _Static_assert on the ABI version, the refusal's status, the size and field offsets of
    wga_maf_index_name, and the two entries assigned to pointers of the documented types"""
    r = subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), "-c",
                        os.path.join(ROOT, "tests", "abi_layout_maf_index.c"), "-o", str(tmp_path / "abi_layout_maf_index.o")],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout


def test_binding_carries_the_two_entries():
    assert len(_lib.PROTOTYPES["wga_maf_index_work_bytes"][1]) == 1
    assert len(_lib.PROTOTYPES["wga_maf_index"][1]) == 18
    dt = engine.MAF_INDEX_NAME_DTYPE
    assert dt.itemsize == 48 and engine.E_FALLBACK == -6
    assert [dt.fields[k][1] for k in ("name_off", "size", "first_line", "n_ivls", "text_off", "name_len", "isref")] == [0, 8, 16, 24, 32, 40, 44]
    assert hasattr(engine.Engine, "maf_index")


def test_library_exports_the_two_entries(emu):
    assert emu.lib.wga_abi_version() == 3
    assert emu.lib.wga_maf_index is not None
    small, big = int(emu.lib.wga_maf_index_work_bytes(0)), int(emu.lib.wga_maf_index_work_bytes(100000))
    assert 0 < small < 65536 and small % 4 == 0 and 100 * 100000 < big < 200 * 100000      # a hundred-odd bytes a line
    assert (emu.get_param("maf_index_hash_bits"), emu.get_param("maf_index_sort_bits")) == (64, 8)


def test_argument_errors(emu):
    k35.check_abi_arguments(emu)


def test_restatement_is_json_and_agrees_with_the_index_restatement():
    """maf_index_ref.index_text parses to what maf_ext_ref.build_index says (the fixtures and a file with escapes), is one line
    without blanks, and keeps the order of first appearance"""
    for name in ("test.maf", "test_chunk_l300.maf"):
        data = open(os.path.join(GOLDEN, name), "rb").read()
        text, err = ref.index_text(data)
        exp, e2 = mref.build_index(data)
        assert err is None and e2 is None
        assert json.loads(text) == exp and list(json.loads(text)) == list(exp)
        assert b"\n" not in text and b" " not in text
    data = k35.HEADER + b"a\ns na\"me\\z 4 2 + 9 AC\ns y 3 2 - 9 A-C\ns c\x01t\x1fl\x7f 0 1 + 9 --A\n\n"
    text, err = ref.index_text(data)
    assert err is None and json.loads(text) == mref.build_index(data)[0]
    assert ref.json_string(b'\x08\x0c\n\r\t"\\\x00\x1f\x7f/') == b'"\\b\\f\\n\\r\\t\\"\\\\\\u0000\\u001f\x7f/"'
    assert ref.interval((1 << 64) - 1, 2, b"-", 7) == b'{"start":18446744073709551615,"end":1,"strand":"-","offset":7}'
    assert ref.index_text(k35.HEADER + b"# nothing\n") == (None, "Empty record")
    # a piece's restatement by hand: two blocks, the second behind two lines
    piece = k35.HEADER + b"a\n" + k35.sline(b"r", 1, 2) + k35.sline(b"x", 3, 4, b"-") + b"\n# c\na\n" + k35.sline(b"r", 10, 5) + b"\n"
    want = ref.piece_index(piece, base=100)
    o2 = 100 + piece.find(b"# c\n")
    assert want["groups"] == [(b"r", 1000, True, 2, [b'{"start":1,"end":3,"strand":"+","offset":116}',
                                                    b'{"start":10,"end":15,"strand":"+","offset":%d}' % o2]),
                              (b"x", 1000, False, 3, [b'{"start":3,"end":7,"strand":"-","offset":116}'])]
    assert (want["n_blocks"], want["n_slines"], want["next_offset"]) == (2, 3, 100 + len(piece))
    later = ref.piece_index(b"#\n" + piece[len(k35.HEADER):], skip=2, base=500, carry=444)
    assert later["groups"][0][4][0].endswith(b'"offset":444}') and later["next_offset"] == 500 + len(piece) - len(k35.HEADER)
