"""The chain reader on the CPU: the C-ABI entry on the emulator build of K23, and the `wgatools` host code linked against it
(tests/emu/wgatools_emu).  Same cases as test_gpu_chain_split.py, plus `--gpus 2` over two emulated devices."""
import pytest

from wgatools_amd import build
import chain_split_cases as cs


@pytest.fixture(scope="module")
def cli():
    return build.build_cli_emu()


@pytest.fixture(scope="module")
def eng(emu):
    return emu


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


@pytest.mark.parametrize("lo", range(0, cs.N_DIFF, 50))
def test_chain2paf_differential(cli, tmp_path, lo):
    cs.check_differential(cli, tmp_path, lo, lo + 50)


def test_chain_commands_over_two_devices(cli, tmp_path, monkeypatch):
    monkeypatch.setenv("WGA_EMU_DEVICES", "2")
    cs.check_gpus(cli, tmp_path, 2)
