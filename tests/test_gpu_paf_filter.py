"""`filter -f paf` on a real GPU: the C-ABI entries (K24) and the `wgatools` binary over libwgahip.so, the cases of
test_emu_paf_filter.py."""
import os
import pytest

from wgatools_amd import build
import paf_filter_cases as pf


pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def cli():
    if not os.path.exists(build.CLI_BIN):
        build.build_cli()
    return build.CLI_BIN


@pytest.fixture(scope="module")
def eng(gpu):
    return gpu


def test_paf_filter_abi_tile_and_group_edges(eng):
    pf.check_abi_tile_and_group_edges(eng)


def test_paf_filter_abi_thresholds(eng):
    pf.check_abi_thresholds(eng)


def test_paf_filter_abi_exactness(eng):
    pf.check_abi_exactness(eng)


@pytest.mark.parametrize("seed", range(12))
def test_paf_filter_abi_random_files(eng, seed):
    pf.check_abi_random_files(eng, [seed])


def test_paf_pairs_abi(eng):
    pf.check_abi_pairs(eng)


@pytest.mark.parametrize("hash_bits", (64, 2))
def test_paf_pairs_abi_large(eng, hash_bits):
    pf.check_abi_pairs_large(eng, hash_bits)


def test_paf_filter_path_selection(cli, tmp_path):
    pf.check_path_selection(cli, tmp_path)


@pytest.mark.parametrize("name", pf.BYTE_FILES)
def test_paf_filter_bytes(cli, tmp_path, name):
    pf.check_bytes(cli, tmp_path, name)


@pytest.mark.parametrize("name", pf.BYTE_FILES)
def test_paf_filter_min_align(cli, tmp_path, name):
    pf.check_min_align(cli, tmp_path, name)


def test_paf_filter_min_align_wraps(cli, tmp_path):
    pf.check_min_align_wraps(cli, tmp_path)


def test_paf_filter_error_order(cli, tmp_path):
    pf.check_error_order(cli, tmp_path)
