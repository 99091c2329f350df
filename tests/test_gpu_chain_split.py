"""The chain reader on a real GPU: the C-ABI entry (K23) and the `wgatools` binary over libwgahip.so, the cases of
test_emu_chain_split.py."""
import os
import pytest

from wgatools_amd import build
import chain_split_cases as cs


pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def cli():
    if not os.path.exists(build.CLI_BIN):
        build.build_cli()
    return build.CLI_BIN


@pytest.fixture(scope="module")
def eng(gpu):
    return gpu


def test_chain_split_abi_tile_and_block_edges(eng):
    cs.check_abi_tile_and_block_edges(eng)


def test_chain_split_abi_tokens(eng):
    cs.check_abi_tokens(eng)


def test_chain_split_abi_order_rules(eng):
    cs.check_abi_order_rules(eng)


def test_chain_split_abi_random_files(eng):
    cs.check_abi_random_files(eng)


def test_chain_split_abi_wide_lines_op_count(eng):
    cs.check_abi_wide_lines_op_count(eng)


def test_chain_reader_selection(cli, tmp_path):
    cs.check_reader_selection(cli, tmp_path)


def test_chain2paf_both_readers(cli, tmp_path):
    cs.check_chain2paf(cli, tmp_path)


def test_chain2maf_both_readers(cli, tmp_path):
    cs.check_chain2maf(cli, tmp_path)


def test_filter_chain_both_readers(cli, tmp_path):
    cs.check_filter(cli, tmp_path)


@pytest.mark.parametrize("lo", range(0, cs.N_DIFF, 10))
def test_chain2paf_differential(cli, tmp_path, lo):
    cs.check_differential(cli, tmp_path, lo, lo + 10)
