"""The row frame writer of `pafpseudo` on a real GPU: the C-ABI entry (K31) and the `wgatools` binary over libwgahip.so, the cases
of test_emu_pseudo_frame.py and the offsets beyond 2^32."""
import os
import pytest

from wgatools_amd import build
import pseudo_frame_cases as k31


pytestmark = pytest.mark.gpu

@pytest.fixture(scope="module")
def cli():
    if not os.path.exists(build.CLI_BIN):
        build.build_cli()
    return build.CLI_BIN


@pytest.fixture(scope="module")
def eng(gpu):
    return gpu


def test_pseudo_frame_abi_alignment_sweep(eng):
    k31.check_abi_alignment_sweep(eng)


def test_pseudo_frame_abi_fills(eng):
    k31.check_abi_fills(eng)


def test_pseudo_frame_abi_tile_borders(eng):
    k31.check_abi_tile_borders(eng)


def test_pseudo_frame_abi_empty_items_at_borders(eng):
    k31.check_abi_empty_items_at_borders(eng)


def test_pseudo_frame_abi_ends(eng):
    k31.check_abi_ends(eng)


@pytest.mark.parametrize("lo", range(0, 12, 4))
def test_pseudo_frame_abi_random(eng, lo):
    k31.check_abi_random(eng, range(lo, lo + 4))


def test_pseudo_frame_abi_bad_items(eng):
    k31.check_abi_bad_items(eng)


def test_pseudo_frame_abi_arguments(eng):
    k31.check_abi_arguments(eng)


def test_pseudo_frame_abi_far_offsets(eng):
    k31.check_abi_far_offsets(eng)


@pytest.mark.parametrize("base", [False, True])
def test_pafpseudo_cli_writers_and_windows(cli, tmp_path, base):
    k31.check_cli_parity(cli, tmp_path, base)


def test_pafpseudo_cli_geometry(cli, tmp_path):
    k31.check_cli_geometry(cli, tmp_path)


def test_pafpseudo_cli_errors_of_a_window(cli, tmp_path):
    k31.check_cli_errors(cli, tmp_path)


def test_pafpseudo_cli_over_two_devices(cli, eng, tmp_path):
    """--gpus 2 where the box has two devices; a box with one refuses the flag before anything is read"""
    if eng.lib.wga_device_count() >= 2:
        k31.check_cli_gpus(cli, tmp_path, 2)
    else:
        paf, fa, recs, contigs = k31.end_to_end_input(tmp_path, False)
        rc, out, err = k31.run(cli, "--gpus", "2", "pafpseudo", str(paf), "-o", str(tmp_path / "out"))
        assert rc == 1 and out == b"" and "only 1 device(s) visible" in err, (rc, out, err)
        assert not os.path.exists(tmp_path / "out")
