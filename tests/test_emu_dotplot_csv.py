"""The base-level csv rows of `dotplot` on the CPU: the C-ABI entry on the emulator build of K26, and the `wgatools` host code
linked against it (tests/emu/wgatools_emu).  Same cases as test_gpu_dotplot_csv.py, plus `--gpus 2` over two emulated devices."""
import pytest

from wgatools_amd import build
import dotplot_csv_cases as dc


@pytest.fixture(scope="module")
def cli():
    return build.build_cli_emu()


@pytest.fixture(scope="module")
def eng(emu):
    return emu


def test_dotplot_csv_abi_block_edges(eng):
    dc.check_abi_block_edges(eng)


def test_dotplot_csv_abi_empty_records(eng):
    dc.check_abi_empty_records(eng)


def test_dotplot_csv_abi_stage_limit(eng):
    dc.check_abi_stage_limit(eng)


def test_dotplot_csv_abi_over_the_stage(eng):
    dc.check_abi_over_the_stage(eng)


def test_dotplot_csv_abi_alignment(eng):
    dc.check_abi_alignment(eng)


def test_dotplot_csv_abi_values(eng):
    dc.check_abi_values(eng)


def test_dotplot_csv_abi_opaque_tails(eng):
    dc.check_abi_opaque_tails(eng)


def test_dotplot_csv_abi_arguments(eng):
    dc.check_abi_arguments(eng)


def test_dotplot_csv_abi_count_fill_consistency(eng):
    dc.check_abi_count_fill(eng)


def test_dotplot_csv_abi_fill_short_total(eng):
    dc.check_abi_fill_short_total(eng)


def test_dotplot_csv_abi_fill_scan_one_off(eng):
    dc.check_abi_fill_scan_one_off(eng)


@pytest.mark.parametrize("lo", range(0, 12, 3))
def test_dotplot_csv_abi_random(eng, lo):
    dc.check_abi_random(eng, range(lo, lo + 3))


def test_dotplot_csv_pipeline_from_k12(eng):
    dc.check_pipeline(eng)


@pytest.mark.parametrize("name", [n for n, _ in dc.GOLDEN_RUNS])
def test_dotplot_csv_cli_golden_both_writers(cli, name):
    dc.check_golden(cli, name)


def test_dotplot_csv_cli_quoted_names(cli, tmp_path):
    dc.check_quoted_names(cli, tmp_path)


def test_dotplot_csv_cli_no_segment(cli, tmp_path):
    dc.check_no_segment(cli, tmp_path)


def test_dotplot_csv_cli_error_leaves_nothing(cli, tmp_path):
    dc.check_error_leaves_nothing(cli, tmp_path)


def test_dotplot_csv_cli_over_two_devices(cli, tmp_path, monkeypatch):
    monkeypatch.setenv("WGA_EMU_DEVICES", "2")
    dc.check_gpus(cli, tmp_path, 2)
