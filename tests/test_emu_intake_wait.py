"""The streaming row kernel's hand-overs of ops and windows (tests/intake_wait_cases.py) on the SIMT emulator."""
import pytest

import intake_wait_cases as ic


@pytest.mark.parametrize("kind", ic.KINDS)
@pytest.mark.parametrize("jt", ic.JOB_TILES)
def test_paf2maf_intake_wait(emu, jt, kind):
    ic.check_paf2maf(emu, jt, kind)


@pytest.mark.parametrize("kind", ic.KINDS)
@pytest.mark.parametrize("jt", ic.JOB_TILES)
def test_pafpseudo_intake_wait(emu, jt, kind):
    ic.check_pafpseudo(emu, jt, kind)
