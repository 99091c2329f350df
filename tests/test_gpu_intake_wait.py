"""The streaming row kernel's hand-overs of ops and windows (tests/intake_wait_cases.py) on a real MI355X, through the C-ABI.
`pytest -m gpu`."""
import pytest

import intake_wait_cases as ic

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("kind", ic.KINDS)
@pytest.mark.parametrize("jt", ic.JOB_TILES)
def test_paf2maf_intake_wait(gpu, jt, kind):
    ic.check_paf2maf(gpu, jt, kind)


@pytest.mark.parametrize("kind", ic.KINDS)
@pytest.mark.parametrize("jt", ic.JOB_TILES)
def test_pafpseudo_intake_wait(gpu, jt, kind):
    ic.check_pafpseudo(gpu, jt, kind)
