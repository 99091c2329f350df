"""`maf-index` on the CPU: the C-ABI entry on the emulator build of K35, and the `wgatools` host code linked against it
(tests/emu/wgatools_emu).  Same cases as test_gpu_maf_index.py."""
import pytest

from wgatools_amd import build
import maf_index_cases as k35


@pytest.fixture(scope="module")
def cli():
    return build.build_cli_emu()


@pytest.fixture(scope="module")
def eng(emu):
    return emu


@pytest.mark.parametrize("counts", (k35.SLINE_COUNTS[:6], k35.SLINE_COUNTS[6:9], k35.SLINE_COUNTS[9:11], k35.SLINE_COUNTS[11:]))
def test_maf_index_abi_sline_counts(eng, counts):
    k35.check_abi_sline_counts(eng, counts)


def test_maf_index_abi_hash_collisions(eng):
    k35.check_abi_hash_collisions(eng)


@pytest.mark.parametrize("groups", ((4, 5, 16), (17, 65)))
def test_maf_index_abi_sort_passes(eng, groups):
    k35.check_abi_sort_passes(eng, groups)


def test_maf_index_abi_offsets(eng):
    k35.check_abi_offsets(eng)


def test_maf_index_abi_numbers(eng):
    k35.check_abi_numbers(eng)


def test_maf_index_abi_errors(eng):
    k35.check_abi_errors(eng)


def test_maf_index_abi_arguments(eng):
    k35.check_abi_arguments(eng)


def test_maf_index_abi_reproducible(eng):
    k35.check_abi_reproducible(eng)


def test_maf_index_abi_random_files(eng):
    k35.check_abi_random(eng, range(3))


def test_maf_index_cli_fixtures(cli, tmp_path):
    k35.check_cli_fixtures(cli, tmp_path)


def test_maf_index_cli_random(cli, tmp_path):
    k35.check_cli_random(cli, tmp_path)


@pytest.mark.parametrize("name", k35.ERROR_FILES)
def test_maf_index_cli_errors_across_pieces(cli, tmp_path, name):
    k35.check_cli_errors_across_pieces(cli, tmp_path, name)


def test_maf_index_cli_fallback_piece(cli, tmp_path):
    k35.check_cli_fallback_piece(cli, tmp_path)


def test_maf_index_cli_loop_closure(cli, tmp_path):
    k35.check_cli_loop_closure(cli, tmp_path)


def test_maf_index_cli_timing_names_the_path(cli, tmp_path):
    k35.check_cli_timing(cli, tmp_path)
