"""The streaming row kernel's record switches, tile borders and restarts (tests/stream_switch_cases.py) on a real MI355X,
through the C-ABI.  `pytest -m gpu`."""
import pytest

import stream_switch_cases as sc

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("jt", sc.JOB_TILES)
def test_paf2maf_stream_switches(gpu, jt):
    sc.check_paf2maf(gpu, jt)


@pytest.mark.parametrize("jt", sc.JOB_TILES)
def test_pafpseudo_stream_switches(gpu, jt):
    sc.check_pafpseudo(gpu, jt)
