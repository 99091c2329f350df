"""The K22 structs of include/wga_hip.h (wga_maf_rewrite_block, wga_maf_rewrite_params) as a C compiler lays them out, against
the numpy dtypes the binding uses (wgatools_amd/engine.py).  No GPU needed."""
import os
import shutil
import subprocess

import pytest

from wgatools_amd.engine import MAF_REWRITE_BLOCK_DTYPE, MAF_REWRITE_PARAMS_DTYPE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_maf_rewrite_struct_layouts(tmp_path):
    cc = shutil.which("cc") or shutil.which("gcc")
    if cc is None:
        pytest.fail("no C compiler")
    src = tmp_path / "l.c"
    fields = [("wga_maf_rewrite_block", MAF_REWRITE_BLOCK_DTYPE, 16), ("wga_maf_rewrite_params", MAF_REWRITE_PARAMS_DTYPE, 40)]
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "wga_hip.h"', "int main(void) {"]
    for name, dt, _ in fields:
        lines.append('printf("%%s %%zu\\n", "%s", sizeof(%s));' % (name, name))
        for f in dt.names:
            lines.append('printf("%%s.%%s %%zu\\n", "%s", "%s", offsetof(%s, %s));' % (name, f, name, f))
    lines.append("return 0; }")
    src.write_text("\n".join(lines))
    exe = str(tmp_path / "l")
    subprocess.run([cc, "-std=c99", "-I" + os.path.join(ROOT, "include"), str(src), "-o", exe], check=True)
    got = dict(l.rsplit(" ", 1) for l in subprocess.run([exe], stdout=subprocess.PIPE, text=True, check=True).stdout.split("\n") if l)
    for name, dt, size in fields:
        assert int(got[name]) == dt.itemsize == size
        for f in dt.names:
            assert int(got["%s.%s" % (name, f)]) == dt.fields[f][1], (name, f)
