"""The csv rows of `dotplot -m overview` on a real GPU: the C-ABI entries (K34) and the `wgatools` binary over libwgahip.so, the
cases of test_emu_dotplot_overview.py."""
import os
import pytest

from wgatools_amd import build
import dotplot_overview_cases as k34


pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def cli():
    if not os.path.exists(build.CLI_BIN):
        build.build_cli()
    return build.CLI_BIN


@pytest.fixture(scope="module")
def eng(gpu):
    return gpu


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


def test_dotplot_overview_cli_over_two_devices(cli, eng, tmp_path):
    """--gpus 2 where the box has two devices; a box with one refuses the flag before anything is read"""
    if eng.lib.wga_device_count() >= 2:
        k34.check_cli_gpus(cli, tmp_path, 2)
    else:
        text, _ = k34.paf_case(5, 20)
        paf = k34.write(tmp_path, "g.paf", text)
        for env in ({}, k34.HOST_WRITER):
            rc, out, err, _ = k34.m2p.timed(cli, ["--gpus", "2", *k34.OVERVIEW, "-f", "paf", paf], env)
            assert rc == 1 and out == b"" and "only 1 device(s) visible" in err, (rc, out, err)
