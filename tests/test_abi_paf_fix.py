"""K29's part of the C-ABI: the layout of wga_paf_fix_sizes is frozen and the binding's dtype agrees with it (no GPU needed)."""
import os
import subprocess

from wgatools_amd import _lib
from wgatools_amd.engine import PAF_FIX_SIZES_DTYPE, PAF_FIX_TILE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_paf_fix_layout_is_frozen(tmp_path):
    r = subprocess.run(["gcc", "-std=c11", "-I" + os.path.join(ROOT, "include"), "-c", os.path.join(ROOT, "tests", "abi_layout_paf_fix.c"),
                        "-o", str(tmp_path / "abi_layout_paf_fix.o")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout


def test_paf_fix_dtype_matches_the_header():
    assert PAF_FIX_SIZES_DTYPE.itemsize == 48
    assert {k: PAF_FIX_SIZES_DTYPE.fields[k][1] for k in PAF_FIX_SIZES_DTYPE.names} == {
        "rows_bytes": 0, "qlist_bytes": 8, "tlist_bytes": 16, "n_records": 24, "n_q_bad": 32, "n_t_bad": 40}
    assert PAF_FIX_TILE == 8192


def test_binding_carries_the_three_entries():
    for name in ("wga_paf_fix_work_bytes", "wga_paf_fix_plan", "wga_paf_fix"):
        assert name in _lib.PROTOTYPES
