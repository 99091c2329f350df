"""`filter` and `rename` on the CPU: the `wgatools` host code linked against the emulator build of K22
(tests/emu/wgatools_emu), and the C-ABI entry on the emulator build.  Same cases as test_gpu_maf_rewrite.py."""
import pytest

from wgatools_amd import build
import maf_rewrite_cases as mr


@pytest.fixture(scope="module")
def cli():
    return build.build_cli_emu()


@pytest.fixture(scope="module")
def eng(emu):
    return emu


def test_rewrite_abi_line_ends_at_tile_edge(eng):
    mr.check_abi_line_ends_at_tile_edge(eng)


def test_rewrite_abi_fields_straddle_tile_edge(eng):
    mr.check_abi_fields_straddle_tile_edge(eng)


def test_rewrite_abi_long_row_between_short_blocks(eng):
    mr.check_abi_long_row_between_short_blocks(eng)


def test_rewrite_abi_many_lines_per_tile(eng):
    mr.check_abi_many_lines_per_tile(eng)


def test_rewrite_abi_thresholds_and_drops(eng):
    mr.check_abi_thresholds(eng)


def test_rewrite_abi_wide_numbers(eng):
    mr.check_abi_wide_numbers(eng)


def test_rewrite_abi_bad_blocks(eng):
    mr.check_abi_bad_blocks(eng)


def test_rewrite_abi_prefixes(eng):
    mr.check_abi_prefixes(eng)


def test_rewrite_abi_random_blocks(eng):
    mr.check_abi_random(eng)


def test_filter_and_rename_fixture(cli):
    mr.check_fixture(cli)


def test_filter_random_files_readers_pieces_windows(cli, tmp_path):
    mr.check_filter_random_files(cli, tmp_path)


def test_rename_random_files_readers_pieces_windows(cli, tmp_path):
    mr.check_rename_random_files(cli, tmp_path)


def test_filter_and_rename_empty_inputs(cli, tmp_path):
    mr.check_empty_inputs(cli, tmp_path)


def test_filter_and_rename_bad_blocks_and_reader_errors(cli, tmp_path):
    mr.check_bad_blocks(cli, tmp_path)


def test_filter_and_rename_argument_errors(cli, tmp_path):
    mr.check_errors(cli, tmp_path)


def test_filter_paf(cli, tmp_path):
    mr.check_paf(cli, tmp_path)


def test_filter_chain(cli, tmp_path):
    mr.check_chain(cli, tmp_path)
