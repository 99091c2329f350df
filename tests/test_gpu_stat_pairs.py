"""The merged table of `stat` on a real GPU: the C-ABI entries (K36) and the `wgatools` binary over libwgahip.so, the cases of
test_emu_stat_pairs.py."""
import os
import pytest

from wgatools_amd import build
import stat_pairs_cases as k36


pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def cli():
    if not os.path.exists(build.CLI_BIN):
        build.build_cli()
    return build.CLI_BIN


@pytest.fixture(scope="module")
def eng(gpu):
    return gpu


@pytest.mark.parametrize("counts", (k36.COUNTS[:8], k36.COUNTS[8:11], k36.COUNTS[11:]))
def test_stat_pairs_abi_record_counts(eng, counts):
    k36.check_abi_record_counts(eng, counts)


def test_stat_pairs_abi_key(eng):
    k36.check_abi_key(eng)


@pytest.mark.parametrize("lo", range(0, 12, 3))
def test_stat_pairs_abi_random_batches(eng, lo):
    k36.check_abi_random(eng, range(lo, lo + 3))


@pytest.mark.parametrize("lo", range(0, 12, 3))
def test_stat_pairs_abi_collisions(eng, lo):
    k36.check_abi_collisions(eng, range(lo, lo + 3))


def test_stat_pairs_abi_wrapped_sums_and_minima(eng):
    k36.check_abi_wrapped(eng)


def test_stat_pairs_abi_fold_order(eng):
    k36.check_abi_fold_order(eng)


def test_stat_pairs_abi_fold_start_and_repeat(eng):
    k36.check_abi_fold_start(eng)


def test_stat_pairs_abi_arguments(eng):
    k36.check_abi_arguments(eng)


@pytest.mark.parametrize("counts", (k36.COUNTS[:8], k36.COUNTS[8:11], k36.COUNTS[11:]))
def test_stat_pair_rows_record_counts(eng, counts):
    k36.check_rows_record_counts(eng, counts)


def test_stat_pair_rows_columns(eng):
    k36.check_rows_columns(eng)


def test_stat_pair_rows_arguments(eng):
    k36.check_rows_arguments(eng)


def test_stat_pair_rows_fill_short_total(eng):
    k36.check_rows_fill_short_total(eng)


def test_stat_pair_rows_fill_row_off_altered(eng):
    k36.check_rows_fill_scan_one_off(eng)


def test_stat_cli_fixtures(cli):
    k36.check_cli_fixtures(cli)


def test_stat_cli_paf(cli, tmp_path):
    k36.check_cli_paf(cli, tmp_path)


def test_stat_cli_empty_and_errors(cli, tmp_path):
    k36.check_cli_empty_and_errors(cli, tmp_path)


def test_stat_cli_maf(cli, tmp_path):
    k36.check_cli_maf(cli, tmp_path)


def test_stat_cli_over_two_devices(cli, eng, tmp_path):
    """--gpus 2 where the box has two devices; a box with one refuses the flag before anything is read"""
    if eng.lib.wga_device_count() >= 2:
        k36.check_cli_gpus(cli, tmp_path, 2)
    else:
        text, _ = k36.paf_case(5, 20)
        paf = k36.write(tmp_path, "g.paf", text)
        for env in ({}, k36.HOST_WRITER):
            rc, out, err = k36.run(cli, "--gpus", "2", "stat", "-f", "paf", paf, env=env)
            assert rc == 1 and out == b"" and "only 1 device(s) visible" in err, (rc, out, err)
