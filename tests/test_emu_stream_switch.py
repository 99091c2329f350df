"""The streaming row kernel's record switches, tile borders and restarts (tests/stream_switch_cases.py) on the SIMT emulator."""
import pytest

import stream_switch_cases as sc


@pytest.mark.parametrize("jt", sc.JOB_TILES)
def test_paf2maf_stream_switches(emu, jt):
    sc.check_paf2maf(emu, jt)


@pytest.mark.parametrize("jt", sc.JOB_TILES)
def test_pafpseudo_stream_switches(emu, jt):
    sc.check_pafpseudo(emu, jt)
