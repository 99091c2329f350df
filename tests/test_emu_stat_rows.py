"""The TSV rows of `stat --each` on the CPU: the C-ABI entries on the emulator build of K33, and the `wgatools` host code linked
against it (tests/emu/wgatools_emu).  Same cases as test_gpu_stat_rows.py, with `--gpus 2` over two emulated devices."""
import pytest

from wgatools_amd import build
import stat_rows_cases as k33


@pytest.fixture(scope="module")
def cli():
    return build.build_cli_emu()


@pytest.fixture(scope="module")
def eng(emu):
    return emu


@pytest.mark.parametrize("counts", (k33.COUNTS[:8], k33.COUNTS[8:11], k33.COUNTS[11:]))
def test_stat_rows_abi_record_counts(eng, counts):
    k33.check_abi_record_counts(eng, counts)


def test_stat_rows_abi_alignment(eng):
    k33.check_abi_alignment(eng)


def test_stat_rows_abi_numbers(eng):
    k33.check_abi_numbers(eng)


def test_stat_rows_abi_wrapped_sums(eng):
    k33.check_abi_wrapped_sums(eng)


def test_stat_rows_abi_names(eng):
    k33.check_abi_names(eng)


def test_stat_rows_abi_floats(eng):
    k33.check_abi_floats(eng)


def test_f32_text_patterns(eng):
    k33.check_f32_text(eng)


def test_stat_rows_abi_arguments(eng):
    k33.check_abi_arguments(eng)


def test_stat_rows_abi_fill_short_total(eng):
    k33.check_abi_fill_short_total(eng)


def test_stat_rows_abi_fill_row_off_altered(eng):
    k33.check_abi_fill_scan_one_off(eng)


@pytest.mark.parametrize("lo", range(0, 12, 3))
def test_stat_rows_abi_random_batches(eng, lo):
    k33.check_abi_random(eng, range(lo, lo + 3))


def test_stat_each_cli_paf(cli, tmp_path):
    k33.check_cli_paf(cli, tmp_path)


def test_stat_each_cli_paf_host_reader(cli, tmp_path):
    k33.check_cli_paf_host_reader(cli, tmp_path)


def test_stat_each_cli_empty_and_errors(cli, tmp_path):
    k33.check_cli_empty_and_errors(cli, tmp_path)


def test_stat_each_cli_maf(cli, tmp_path):
    k33.check_cli_maf(cli, tmp_path)


def test_stat_each_cli_over_two_devices(cli, tmp_path, monkeypatch):
    monkeypatch.setenv("WGA_EMU_DEVICES", "2")
    k33.check_cli_gpus(cli, tmp_path, 2)
