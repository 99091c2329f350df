"""`filter -f chain` on a real GPU: the C-ABI entry (K25) and the `wgatools` binary over libwgahip.so, the cases of
test_emu_chain_filter.py."""
import os
import pytest

from wgatools_amd import build
import chain_filter_cases as cf


pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def cli():
    if not os.path.exists(build.CLI_BIN):
        build.build_cli()
    return build.CLI_BIN


@pytest.fixture(scope="module")
def eng(gpu):
    return gpu


def test_chain_filter_abi_fill_block_edges(eng):
    cf.check_abi_fill_block_edges(eng)


def test_chain_filter_abi_stage_limit(eng):
    cf.check_abi_stage_limit(eng)


def test_chain_filter_abi_over_the_stage(eng):
    cf.check_abi_over_the_stage(eng)


def test_chain_filter_abi_plan_edges(eng):
    cf.check_abi_plan_edges(eng)


def test_chain_filter_abi_alignment(eng):
    cf.check_abi_alignment(eng)


def test_chain_filter_abi_thresholds(eng):
    cf.check_abi_thresholds(eng)


def test_chain_filter_abi_values(eng):
    cf.check_abi_values(eng)


def test_chain_filter_abi_hand_built_arrays(eng):
    cf.check_abi_hand_built(eng)


def test_chain_filter_abi_arguments(eng):
    cf.check_abi_arguments(eng)


def test_chain_filter_abi_count_fill_consistency(eng):
    cf.check_abi_count_fill(eng)


def test_chain_filter_abi_fill_short_total(eng):
    cf.check_abi_fill_short_total(eng)


def test_chain_filter_abi_fill_scan_one_off(eng):
    cf.check_abi_fill_scan_one_off(eng)


@pytest.mark.parametrize("lo", range(0, 12, 3))
def test_chain_filter_abi_random_files(eng, lo):
    cf.check_abi_random_files(eng, range(lo, lo + 3))


@pytest.mark.parametrize("part", range(cf.PATH_PARTS))
def test_chain_filter_path_selection(cli, tmp_path, part):
    cf.check_path_selection(cli, tmp_path, part)


@pytest.mark.parametrize("name", cf.BYTE_FILES)
def test_chain_filter_bytes(cli, tmp_path, name):
    cf.check_bytes(cli, tmp_path, name)


def test_chain_filter_error_order(cli, tmp_path):
    cf.check_error_order(cli, tmp_path)
