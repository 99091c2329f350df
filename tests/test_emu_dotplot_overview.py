"""The csv rows of `dotplot -m overview` on the CPU: the C-ABI entries on the emulator build of K34, and the `wgatools` host code
linked against it (tests/emu/wgatools_emu).  Same cases as test_gpu_dotplot_overview.py, with `--gpus 2` and `--gpus 3` over
emulated devices."""
import pytest

from wgatools_amd import build
import dotplot_overview_cases as k34


@pytest.fixture(scope="module")
def cli():
    return build.build_cli_emu()


@pytest.fixture(scope="module")
def eng(emu):
    return emu


@pytest.mark.parametrize("counts", (k34.COUNTS[:8], k34.COUNTS[8:11], k34.COUNTS[11:]))
def test_dotplot_overview_abi_record_counts(eng, counts):
    k34.check_abi_record_counts(eng, counts)


def test_dotplot_overview_abi_alignment(eng):
    k34.check_abi_alignment(eng)


def test_dotplot_overview_abi_numbers(eng):
    k34.check_abi_numbers(eng)


def test_dotplot_overview_abi_identity(eng):
    k34.check_abi_identity(eng)


def test_dotplot_overview_abi_names(eng):
    k34.check_abi_names(eng)


def test_f64_text_patterns(eng):
    k34.check_f64_text(eng)


def test_dotplot_overview_abi_arguments(eng):
    k34.check_abi_arguments(eng)


def test_dotplot_overview_abi_fill_short_total(eng):
    k34.check_abi_fill_short_total(eng)


def test_dotplot_overview_abi_fill_row_off_altered(eng):
    k34.check_abi_fill_scan_one_off(eng)


@pytest.mark.parametrize("lo", range(0, 12, 3))
def test_dotplot_overview_abi_random_batches(eng, lo):
    k34.check_abi_random(eng, range(lo, lo + 3))


def test_dotplot_overview_cli_paf(cli, tmp_path):
    k34.check_cli_paf(cli, tmp_path)


def test_dotplot_overview_cli_paf_host_reader(cli, tmp_path):
    k34.check_cli_paf_host_reader(cli, tmp_path)


def test_dotplot_overview_cli_empty_and_errors(cli, tmp_path):
    k34.check_cli_empty_and_errors(cli, tmp_path)


def test_dotplot_overview_cli_maf(cli, tmp_path):
    k34.check_cli_maf(cli, tmp_path)


@pytest.mark.parametrize("gpus", (2, 3))
def test_dotplot_overview_cli_over_devices(cli, tmp_path, monkeypatch, gpus):
    monkeypatch.setenv("WGA_EMU_DEVICES", str(gpus))
    k34.check_cli_gpus(cli, tmp_path, gpus)
