"""The chain heads of `paf2chain` / `maf2chain` on the CPU: the C-ABI entry on the emulator build of K30, and the `wgatools` host
code linked against it (tests/emu/wgatools_emu).  Same cases as test_gpu_chain_heads.py, with `--gpus 2` over two emulated
devices."""
import pytest

from wgatools_amd import build
import chain_heads_cases as k30


@pytest.fixture(scope="module")
def cli():
    return build.build_cli_emu()


@pytest.fixture(scope="module")
def eng(emu):
    return emu


@pytest.mark.parametrize("counts", (k30.COUNTS[:5], k30.COUNTS[5:8], k30.COUNTS[8:]))
def test_chain_heads_abi_record_counts(eng, counts):
    k30.check_abi_record_counts(eng, counts)


def test_chain_heads_abi_heads_only(eng):
    k30.check_abi_heads_only(eng)


def test_chain_heads_abi_alignment(eng):
    k30.check_abi_alignment(eng)


def test_chain_heads_abi_names(eng):
    k30.check_abi_names(eng)


def test_chain_heads_abi_values(eng):
    k30.check_abi_values(eng)


def test_chain_heads_abi_minus_quirk(eng):
    k30.check_abi_minus_quirk(eng)


def test_chain_heads_abi_bad_records(eng):
    k30.check_abi_bad_records(eng)


def test_chain_heads_abi_bad_records_far(eng):
    k30.check_abi_bad_records_far(eng)


def test_chain_heads_abi_hand_built_arrays(eng):
    k30.check_abi_hand_built(eng)


def test_chain_heads_abi_long_records(eng):
    k30.check_abi_long_records(eng)


def test_chain_heads_abi_arguments(eng):
    k30.check_abi_arguments(eng)


@pytest.mark.parametrize("lo", range(0, 12, 3))
def test_chain_heads_abi_random_batches(eng, lo):
    k30.check_abi_random(eng, range(lo, lo + 3))


def test_paf2chain_cli_device_writer(cli, tmp_path):
    k30.check_cli_paf2chain(cli, tmp_path)


def test_paf2chain_cli_host_reader(cli, tmp_path):
    k30.check_cli_paf2chain_host_reader(cli, tmp_path)


def test_paf2chain_cli_pieces_and_invalid_op(cli, tmp_path):
    k30.check_cli_paf2chain_pieces(cli, tmp_path)


def test_maf2chain_cli_device_writer(cli, tmp_path):
    k30.check_cli_maf2chain(cli, tmp_path)


def test_maf2chain_cli_query_name(cli, tmp_path):
    k30.check_cli_maf2chain_query_name(cli, tmp_path)


def test_chain_heads_cli_over_two_devices(cli, tmp_path, monkeypatch):
    monkeypatch.setenv("WGA_EMU_DEVICES", "2")
    k30.check_cli_gpus(cli, tmp_path, 2)
