"""`maf-index` and `maf-ext` on a real GPU: the `wgatools` binary over libwgahip.so (K21) and the C-ABI entry,
the cases of test_emu_maf_ext.py (the long block ten times as long)."""
import os
import pytest

from wgatools_amd import build
import maf_ext_cases as mx


pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def cli():
    if not os.path.exists(build.CLI_BIN):
        build.build_cli()
    return build.CLI_BIN


@pytest.fixture(scope="module")
def eng(gpu):
    return gpu


def test_ext_literal_cases(cli, tmp_path):
    mx.check_literal(cli, tmp_path)


def test_index_fixtures(cli, tmp_path):
    mx.check_index_fixtures(cli, tmp_path)


def test_index_random_files_pieces_and_readers(cli, tmp_path):
    mx.check_index_random(cli, tmp_path)


def test_index_errors_output_and_escaping(cli, tmp_path):
    mx.check_index_errors_and_output(cli, tmp_path)


def test_index_refuses_compressed_input(cli, tmp_path):
    mx.check_index_refuses_compressed(cli, tmp_path)


def test_index_then_call_contigs(cli, tmp_path):
    mx.check_index_then_call(cli, tmp_path)


def test_ext_random_battery(cli, tmp_path):
    mx.check_battery(cli, tmp_path)


def test_ext_outputs_windows_and_readers(cli, tmp_path):
    mx.check_ext_outputs_and_windows(cli, tmp_path)


def test_ext_non_ascii_rows_on_the_host(cli, tmp_path):
    mx.check_ext_non_ascii(cli, tmp_path)


def test_ext_short_row_panics_behind_the_records_in_front(cli, tmp_path):
    mx.check_ext_short_row(cli, tmp_path)


def test_ext_errors(cli, tmp_path):
    mx.check_ext_errors(cli, tmp_path)


def test_ext_foreign_index(cli, tmp_path):
    mx.check_ext_foreign_index(cli, tmp_path)


def test_ext_hand_written_index(cli, tmp_path):
    mx.check_ext_hand_written_index(cli, tmp_path)


def test_slice_abi_empty_and_all_gap_rows(eng):
    mx.check_abi_empty(eng)
    mx.check_abi_all_gap_rows(eng)


def test_slice_abi_widths_and_boundaries(eng):
    mx.check_abi_widths(eng)


def test_slice_abi_long_gap_run(eng):
    mx.check_abi_long_gap_run(eng)


def test_slice_abi_many_hits_one_block(eng):
    mx.check_abi_many_hits_one_block(eng)


def test_slice_abi_tile_edges_and_wide_numbers(eng):
    mx.check_abi_tile_edges(eng)


def test_slice_abi_short_rows(eng):
    mx.check_abi_short_rows(eng)


def test_slice_abi_long_block(eng):
    mx.check_abi_long_block(eng, cols=10 ** 7)
