"""The TSV rows of `stat --each` on a real GPU: the C-ABI entries (K33) and the `wgatools` binary over libwgahip.so, the cases of
test_emu_stat_rows.py."""
import os
import pytest

from wgatools_amd import build
import stat_rows_cases as k33


pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def cli():
    if not os.path.exists(build.CLI_BIN):
        build.build_cli()
    return build.CLI_BIN


@pytest.fixture(scope="module")
def eng(gpu):
    return gpu


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


def test_stat_each_cli_over_two_devices(cli, eng, tmp_path):
    """--gpus 2 where the box has two devices; a box with one refuses the flag before anything is read"""
    if eng.lib.wga_device_count() >= 2:
        k33.check_cli_gpus(cli, tmp_path, 2)
    else:
        text, _ = k33.paf_case(5, 20)
        paf = k33.write(tmp_path, "g.paf", text)
        for env in ({}, k33.HOST_WRITER):
            rc, out, err = k33.run(cli, "--gpus", "2", "stat", "-f", "paf", "-e", paf, env=env)
            assert rc == 1 and out == b"" and "only 1 device(s) visible" in err, (rc, out, err)
