"""The MAF record frames of `paf2maf` / `chain2maf` on the CPU: the C-ABI entry on the emulator build of K32, and the `wgatools`
host code linked against it (tests/emu/wgatools_emu).  Same cases as test_gpu_maf_frame.py (but the fill beyond 4 GiB, which needs
a GPU's memory), with `--gpus 2` over two emulated devices."""
import pytest

from wgatools_amd import build
import maf_frame_cases as k32


@pytest.fixture(scope="module")
def cli():
    return build.build_cli_emu()


@pytest.fixture(scope="module")
def eng(emu):
    return emu


@pytest.mark.parametrize("counts", (k32.COUNTS[:8], k32.COUNTS[8:11], k32.COUNTS[11:]))
def test_maf_frame_abi_record_counts(eng, counts):
    k32.check_abi_record_counts(eng, counts)


def test_maf_frame_abi_either_order(eng):
    k32.check_abi_either_order(eng)


def test_maf_frame_abi_alignment(eng):
    k32.check_abi_alignment(eng)


def test_maf_frame_abi_empty_rows(eng):
    k32.check_abi_empty_rows(eng)


def test_maf_frame_abi_names(eng):
    k32.check_abi_names(eng)


def test_maf_frame_abi_values(eng):
    k32.check_abi_values(eng)


def test_maf_frame_abi_layout_equivalence(eng):
    k32.check_abi_layout_equivalence(eng)


def test_maf_frame_abi_far_places_count(eng):
    k32.check_abi_far_places_count(eng)


@pytest.mark.parametrize("n", (9, 300, 1030))
def test_maf_frame_abi_bad_records_by_hand(eng, n):
    k32.check_abi_bad_records_by_hand(eng, (n,))


def test_maf_frame_abi_bad_records_pipeline(eng):
    k32.check_abi_bad_records_pipeline(eng)


def test_maf_frame_abi_arguments(eng):
    k32.check_abi_arguments(eng)


@pytest.mark.parametrize("lo", range(0, 12, 3))
def test_maf_frame_abi_random_batches(eng, lo):
    k32.check_abi_random(eng, range(lo, lo + 3))


def test_paf2maf_cli_both_writers(cli, tmp_path):
    k32.check_cli_paf2maf(cli, tmp_path)


def test_paf2maf_cli_host_reader(cli, tmp_path):
    k32.check_cli_paf2maf_host_reader(cli, tmp_path)


def test_paf2maf_cli_pieces_and_errors(cli, tmp_path):
    k32.check_cli_paf2maf_pieces(cli, tmp_path)


def test_chain2maf_cli_both_writers(cli, tmp_path):
    k32.check_cli_chain2maf(cli, tmp_path)


def test_maf_frame_cli_over_two_devices(cli, tmp_path, monkeypatch):
    monkeypatch.setenv("WGA_EMU_DEVICES", "2")
    k32.check_cli_gpus(cli, tmp_path, 2)
