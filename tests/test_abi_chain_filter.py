"""K25's part of the C-ABI: the layout of wga_chain_filter_params is frozen, the ABI version stays 3 and the binding's dtype
agrees with the header (no GPU needed)."""
import os
import subprocess

from wgatools_amd import _lib
from wgatools_amd import engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_chain_filter_layout_is_frozen(tmp_path):
    r = subprocess.run(["gcc", "-std=c11", "-I" + os.path.join(ROOT, "include"), "-c", os.path.join(ROOT, "tests", "abi_layout_chain_filter.c"),
                        "-o", str(tmp_path / "abi_layout_chain_filter.o")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout


def test_chain_filter_dtype_matches_the_header():
    dt = engine.CHAIN_FILTER_PARAMS_DTYPE
    assert dt.itemsize == 16
    assert {k: dt.fields[k][1] for k in dt.names} == {"min_block_size": 0, "min_query_size": 8}


def test_binding_carries_the_two_entries():
    for name in ("wga_chain_filter_work_bytes", "wga_chain_filter"):
        assert name in _lib.PROTOTYPES
    assert hasattr(engine.Engine, "chain_filter")
