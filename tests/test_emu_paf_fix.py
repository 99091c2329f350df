"""`validate --fix` on the CPU: the C-ABI entries on the emulator build of K29, and the `wgatools` host code linked against it
(tests/emu/wgatools_emu).  Same cases as test_gpu_paf_fix.py, plus the restatement's own properties."""
import pytest

from wgatools_amd import build
import cli_cases
import paf_fix_cases as pf


@pytest.fixture(scope="module")
def cli():
    return build.build_cli_emu()


@pytest.fixture(scope="module")
def eng(emu):
    return emu


def test_reference_properties():
    pf.check_reference_properties()


def test_paf_fix_abi_digit_counts(eng):
    pf.check_abi_digit_counts(eng)


def test_paf_fix_abi_tile_and_group_edges(eng):
    pf.check_abi_tile_and_group_edges(eng)


def test_paf_fix_abi_lists(eng):
    pf.check_abi_lists(eng)


def test_paf_fix_abi_untaken(eng):
    pf.check_abi_untaken(eng)


@pytest.mark.parametrize("lo", range(0, 12, 2))
def test_paf_fix_abi_random_files(eng, lo):
    pf.check_abi_random_files(eng, range(lo, lo + 2))


@pytest.mark.parametrize("part", pf.PATH_PARTS)
def test_validate_fix_path_selection(cli, tmp_path, part):
    pf.check_path_selection(cli, tmp_path, part)


@pytest.mark.parametrize("name", pf.BYTE_FILES)
def test_validate_fix_bytes(cli, tmp_path, name):
    pf.check_bytes(cli, tmp_path, name)


def test_validate_fix_four_row_case(cli, tmp_path):
    cli_cases.test_validate_report_and_fix(cli, tmp_path)       # its cs:Z: row makes it a host piece: the bytes it always gave


def test_validate_fix_alternation(cli, tmp_path):
    pf.check_alternation(cli, tmp_path)


def test_validate_fix_errors(cli, tmp_path):
    pf.check_errors(cli, tmp_path)
