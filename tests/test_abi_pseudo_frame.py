"""K31's part of the C-ABI: the entry, its item and the four kinds stand in the header, in the binding and in the library, the ABI
version stays 3, and the argument errors of wga_pafpseudo_frame (on the emulator build: no GPU needed)."""
import os
import re
import subprocess

from wgatools_amd import _lib
from wgatools_amd import engine
import pseudo_frame_cases as k31

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_declares_the_entry():
    text = open(os.path.join(ROOT, "include", "wga_hip.h")).read()
    assert re.search(r"#define WGA_ABI_VERSION 3\b", text)
    for name, value in (("FILL", 0), ("COPY_POOL", 1), ("COPY_TEXT", 2), ("HOLE", 3)):
        assert re.search(r"#define WGA_SPAN_%s\s+%du\b" % (name, value), text), name
    assert re.search(r"typedef struct \{ uint64_t dst, len, src; uint32_t kind, pad; \} wga_span_item;", text)
    assert re.search(r"int wga_pafpseudo_frame\(wga_ctx\*, uint64_t n_items, const wga_span_item\* d_items,\s+"
                     r"const uint8_t\* d_pool, uint64_t pool_bytes,\s+const uint8_t\* d_text, uint64_t text_bytes,\s+"
                     r"uint8_t\* d_out, uint64_t out_bytes, uint64_t\* d_first_bad\);", text)
    assert "pseudomaf.rs:98-209" in text
    tile = re.search(r"#define WGA_PSEUDO_FRAME_TILE (\d+)u\b", text)
    assert tile and int(tile.group(1)) == engine.PSEUDO_FRAME_TILE                 # the tests aim at the borders of this tile


def test_layout_and_prototype(tmp_path):
    """tests/abi_layout_pseudo_frame.c: _Static_assert on the ABI version, the item's 32 bytes and the kinds, and the entry assigned
    to a pointer of the documented type"""
    r = subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), "-c",
                        os.path.join(ROOT, "tests", "abi_layout_pseudo_frame.c"), "-o", str(tmp_path / "abi_layout_pseudo_frame.o")],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout


def test_binding_carries_the_entry():
    assert len(_lib.PROTOTYPES["wga_pafpseudo_frame"][1]) == 10
    assert engine.SPAN_ITEM_DTYPE.itemsize == 32
    assert [engine.SPAN_ITEM_DTYPE.fields[k][1] for k in ("dst", "len", "src", "kind", "pad")] == [0, 8, 16, 24, 28]
    assert (engine.SPAN_FILL, engine.SPAN_COPY_POOL, engine.SPAN_COPY_TEXT, engine.SPAN_HOLE) == (0, 1, 2, 3)
    assert hasattr(engine.Engine, "pafpseudo_frame")


def test_library_exports_the_entry(emu):
    assert emu.lib.wga_abi_version() == 3
    assert emu.lib.wga_pafpseudo_frame is not None


def test_argument_errors(emu):
    k31.check_abi_arguments(emu)
