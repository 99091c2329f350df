"""`chain2paf` on a real GPU: the C-ABI entry (K27) and the `wgatools` binary over libwgahip.so, the cases of
test_emu_chain2paf.py."""
import os
import pytest

from wgatools_amd import build
import chain2paf_cases as c2p


pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def cli():
    if not os.path.exists(build.CLI_BIN):
        build.build_cli()
    return build.CLI_BIN


@pytest.fixture(scope="module")
def eng(gpu):
    return gpu


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


def test_chain2paf_path_under_two_gpus(cli, eng, tmp_path):
    """--gpus 2 keeps the host writer; a box with one device refuses the flag before any path is chosen"""
    path = c2p.write(tmp_path, "g.chain", c2p.random_file(5)[2])
    rc, out, err = c2p.run(cli, "--gpus", "2", "__chain2paf_path", path)
    if eng.lib.wga_device_count() >= 2:
        assert (rc, out.strip()) == (0, b"host"), err
    else:
        assert rc == 1 and "only 1 device(s) visible" in err, (rc, out, err)
