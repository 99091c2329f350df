"""K24's part of the C-ABI: the layouts of wga_paf_pair and wga_paf_filter_params are frozen and the binding's dtypes agree with
them (no GPU needed)."""
import os
import subprocess

from wgatools_amd import _lib
from wgatools_amd.engine import PAF_FILTER_PARAMS_DTYPE, PAF_FILTER_TILE, PAF_PAIR_DTYPE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_paf_filter_layouts_are_frozen(tmp_path):
    r = subprocess.run(["gcc", "-std=c11", "-I" + os.path.join(ROOT, "include"), "-c", os.path.join(ROOT, "tests", "abi_layout_paf_filter.c"),
                        "-o", str(tmp_path / "abi_layout_paf_filter.o")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout


def test_paf_filter_dtypes_match_the_header():
    assert PAF_PAIR_DTYPE.itemsize == 40
    assert {k: PAF_PAIR_DTYPE.fields[k][1] for k in PAF_PAIR_DTYPE.names} == {
        "first_line": 0, "sum": 8, "qname_off": 16, "tname_off": 24, "qname_len": 32, "tname_len": 36}
    assert PAF_FILTER_PARAMS_DTYPE.itemsize == 32
    assert {k: PAF_FILTER_PARAMS_DTYPE.fields[k][1] for k in PAF_FILTER_PARAMS_DTYPE.names} == {
        "min_block_size": 0, "min_query_size": 8, "d_pair_of_line": 16, "d_pair_keep": 24}
    assert PAF_FILTER_TILE == 8192


def test_binding_carries_the_four_entries():
    for name in ("wga_paf_pairs_work_bytes", "wga_paf_pairs", "wga_paf_filter_work_bytes", "wga_paf_filter"):
        assert name in _lib.PROTOTYPES
