"""`maf2paf` on a real GPU: the C-ABI entry (K28) and the `wgatools` binary over libwgahip.so, the cases of
test_emu_maf2paf.py."""
import os
import pytest

from wgatools_amd import build
import maf2paf_cases as m2p


pytestmark = pytest.mark.gpu

@pytest.fixture(scope="module")
def cli():
    if not os.path.exists(build.CLI_BIN):
        build.build_cli()
    return build.CLI_BIN


@pytest.fixture(scope="module")
def eng(gpu):
    return gpu


def test_maf2paf_abi_fill_block_edges(eng):
    m2p.check_abi_fill_block_edges(eng)


def test_maf2paf_abi_plan_edges(eng):
    m2p.check_abi_plan_edges(eng)


def test_maf2paf_abi_stage_limit(eng):
    m2p.check_abi_stage_limit(eng)


def test_maf2paf_abi_over_the_stage(eng):
    m2p.check_abi_over_the_stage(eng)


def test_maf2paf_abi_values(eng):
    m2p.check_abi_values(eng)


def test_maf2paf_abi_quoting(eng):
    m2p.check_abi_quoting(eng)


def test_maf2paf_abi_cigar_is_k11s(eng):
    m2p.check_abi_cross_k11(eng)


def test_maf2paf_abi_hand_built_arrays(eng):
    m2p.check_abi_hand_built(eng)


def test_maf2paf_abi_alignment(eng):
    m2p.check_abi_alignment(eng)


def test_maf2paf_abi_count_fill_consistency(eng):
    m2p.check_abi_count_fill(eng)


def test_maf2paf_abi_fill_short_total(eng):
    m2p.check_abi_fill_short_total(eng)


def test_maf2paf_abi_fill_scan_one_off(eng):
    m2p.check_abi_fill_scan_one_off(eng)


def test_maf2paf_abi_arguments(eng):
    m2p.check_abi_arguments(eng)


@pytest.mark.parametrize("lo", range(0, 12, 3))
def test_maf2paf_abi_random_files(eng, lo):
    m2p.check_abi_random_files(eng, range(lo, lo + 3))


def test_maf2paf_cli_fixture(cli):
    m2p.check_cli_fixture(cli)


def test_maf2paf_cli_random_file(cli, tmp_path):
    m2p.check_cli_random(cli, tmp_path)


def test_maf2paf_cli_quoted_name(cli, tmp_path):
    m2p.check_cli_quoted(cli, tmp_path)


def test_maf2paf_cli_host_reader(cli, tmp_path):
    m2p.check_cli_host_reader(cli, tmp_path)


def test_maf2paf_cli_query_name(cli, tmp_path):
    m2p.check_cli_query_name(cli, tmp_path)


def test_maf2paf_cli_pieces(cli, tmp_path):
    m2p.check_cli_pieces(cli, tmp_path)


def test_maf2paf_cli_over_two_devices(cli, eng, tmp_path):
    """--gpus 2 where the box has two devices; a box with one refuses the flag before anything is read"""
    if eng.lib.wga_device_count() >= 2:
        m2p.check_cli_gpus(cli, tmp_path, 2)
    else:
        path = m2p.write(tmp_path, "g.maf", m2p.random_maf(9)[0])
        rc, out, err = m2p.run(cli, "--gpus", "2", "maf2paf", path)
        assert rc == 1 and out == b"" and "only 1 device(s) visible" in err, (rc, out, err)
