"""`chain2paf` on the CPU: the C-ABI entry on the emulator build of K27, and the `wgatools` host code linked against it
(tests/emu/wgatools_emu).  Same cases as test_gpu_chain2paf.py, plus `--gpus 2` over two emulated devices."""
import pytest

from wgatools_amd import build
import chain2paf_cases as c2p


@pytest.fixture(scope="module")
def cli():
    return build.build_cli_emu()


@pytest.fixture(scope="module")
def eng(emu):
    return emu


def test_chain2paf_abi_fill_block_edges(eng):
    c2p.check_abi_fill_block_edges(eng)


def test_chain2paf_abi_plan_edges(eng):
    c2p.check_abi_plan_edges(eng)


def test_chain2paf_abi_sums_across_blocks(eng):
    c2p.check_abi_sums_across_blocks(eng)


def test_chain2paf_abi_stage_limit(eng):
    c2p.check_abi_stage_limit(eng)


def test_chain2paf_abi_over_the_stage(eng):
    c2p.check_abi_over_the_stage(eng)


def test_chain2paf_abi_values(eng):
    c2p.check_abi_values(eng)


def test_chain2paf_abi_quoting(eng):
    c2p.check_abi_quoting(eng)


def test_chain2paf_abi_hand_built_arrays(eng):
    c2p.check_abi_hand_built(eng)


def test_chain2paf_abi_alignment(eng):
    c2p.check_abi_alignment(eng)


def test_chain2paf_abi_count_fill_consistency(eng):
    c2p.check_abi_count_fill(eng)


def test_chain2paf_abi_fill_short_total(eng):
    c2p.check_abi_fill_short_total(eng)


def test_chain2paf_abi_fill_scan_one_off(eng):
    c2p.check_abi_fill_scan_one_off(eng)


def test_chain2paf_abi_arguments(eng):
    c2p.check_abi_arguments(eng)


@pytest.mark.parametrize("lo", range(0, 12, 3))
def test_chain2paf_abi_random_files(eng, lo):
    c2p.check_abi_random_files(eng, range(lo, lo + 3))


@pytest.mark.parametrize("name", c2p.BYTE_FILES)
def test_chain2paf_bytes(cli, tmp_path, name):
    c2p.check_bytes(cli, tmp_path, name)


def test_chain2paf_path_selection(cli, tmp_path):
    c2p.check_path_selection(cli, tmp_path)


def test_chain2paf_wide_values_keep_the_host_writer(cli, tmp_path):
    c2p.check_wide_values(cli, tmp_path)


def test_chain2paf_timing_phase(cli, tmp_path):
    c2p.check_timing_phase(cli, tmp_path)


def test_chain2paf_over_two_devices(cli, tmp_path, monkeypatch):
    monkeypatch.setenv("WGA_EMU_DEVICES", "2")
    c2p.check_gpus(cli, tmp_path, 2)
