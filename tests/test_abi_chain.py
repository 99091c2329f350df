"""The chain reader's part of the C-ABI: the head's layout is frozen and the binding's dtype agrees with it (no GPU needed)."""
import os
import subprocess

from wgatools_amd.engine import CHAIN_HEAD_DTYPE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_chain_head_layout_is_frozen(tmp_path):
    r = subprocess.run(["gcc", "-std=c11", "-I" + os.path.join(ROOT, "include"), "-c", os.path.join(ROOT, "tests", "abi_layout_chain.c"),
                        "-o", str(tmp_path / "abi_layout_chain.o")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout


def test_chain_head_dtype_matches_the_header():
    assert CHAIN_HEAD_DTYPE.itemsize == 96
    assert {k: CHAIN_HEAD_DTYPE.fields[k][1] for k in CHAIN_HEAD_DTYPE.names} == {
        "num": 0, "tname_off": 64, "qname_off": 72, "tname_len": 80, "qname_len": 84, "tstrand_neg": 88, "qstrand_neg": 89, "pad": 90}
