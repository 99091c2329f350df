"""`wgatools --gpus N filter` / `rename` on CPU: the host layer linked against the emulator build, which reports
WGA_EMU_DEVICES devices.  Each device takes a contiguous range of a piece's blocks; the bytes are those of `--gpus 1`, and a
bad block ends the output in front of it whichever device owns it."""
import pytest

import maf_rewrite_cases as mr
from wgatools_amd import build


@pytest.fixture(scope="module")
def cli():
    return build.build_cli_emu()


def test_filter_and_rename_ranges_per_device(cli, tmp_path, monkeypatch):
    monkeypatch.setenv("WGA_EMU_DEVICES", "3")
    mr.check_gpus(cli, tmp_path, (2, 3))
