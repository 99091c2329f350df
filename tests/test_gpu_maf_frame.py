"""The MAF record frames of `paf2maf` / `chain2maf` on a real GPU: the C-ABI entry (K32) and the `wgatools` binary over
libwgahip.so, the cases of test_emu_maf_frame.py and the fill beyond 4 GiB."""
import os
import pytest

from wgatools_amd import build
import maf_frame_cases as k32


pytestmark = pytest.mark.gpu

@pytest.fixture(scope="module")
def cli():
    if not os.path.exists(build.CLI_BIN):
        build.build_cli()
    return build.CLI_BIN


@pytest.fixture(scope="module")
def eng(gpu):
    return gpu


@pytest.mark.parametrize("counts", (k32.COUNTS[:8], k32.COUNTS[8:11], k32.COUNTS[11:]))
def test_maf_frame_abi_record_counts(eng, counts):
    k32.check_abi_record_counts(eng, counts)


def test_maf_frame_abi_either_order(eng):
    k32.check_abi_either_order(eng)


def test_maf_frame_abi_alignment(eng):
    k32.check_abi_alignment(eng)


def test_maf_frame_abi_empty_rows(eng):
    k32.check_abi_empty_rows(eng)


def test_maf_frame_abi_names(eng):
    k32.check_abi_names(eng)


def test_maf_frame_abi_values(eng):
    k32.check_abi_values(eng)


def test_maf_frame_abi_layout_equivalence(eng):
    k32.check_abi_layout_equivalence(eng)


def test_maf_frame_abi_far_places_count(eng):
    k32.check_abi_far_places_count(eng)


def test_maf_frame_abi_far_places_fill(eng):
    k32.check_abi_far_places_fill(eng)


@pytest.mark.parametrize("n", (9, 300, 1030))
def test_maf_frame_abi_bad_records_by_hand(eng, n):
    k32.check_abi_bad_records_by_hand(eng, (n,))


def test_maf_frame_abi_bad_records_pipeline(eng):
    k32.check_abi_bad_records_pipeline(eng)


def test_maf_frame_abi_arguments(eng):
    k32.check_abi_arguments(eng)


@pytest.mark.parametrize("lo", range(0, 12, 3))
def test_maf_frame_abi_random_batches(eng, lo):
    k32.check_abi_random(eng, range(lo, lo + 3))


def test_paf2maf_cli_both_writers(cli, tmp_path):
    k32.check_cli_paf2maf(cli, tmp_path)


def test_paf2maf_cli_host_reader(cli, tmp_path):
    k32.check_cli_paf2maf_host_reader(cli, tmp_path)


def test_paf2maf_cli_pieces_and_errors(cli, tmp_path):
    k32.check_cli_paf2maf_pieces(cli, tmp_path)


def test_chain2maf_cli_both_writers(cli, tmp_path):
    k32.check_cli_chain2maf(cli, tmp_path)


def test_maf_frame_cli_over_two_devices(cli, eng, tmp_path):
    """--gpus 2 where the box has two devices; a box with one refuses the flag before anything is read"""
    if eng.lib.wga_device_count() >= 2:
        k32.check_cli_gpus(cli, tmp_path, 2)
    else:
        recs, t_fa, q_fa = k32.paf_case(tmp_path, 6, 80)
        paf = k32.write(tmp_path, "g.paf", k32.paf_text(recs))
        crecs, ct_fa, cq_fa = k32.chain_case(tmp_path, 8, 60)
        ch = k32.write(tmp_path, "g.chain", k32.chain_text(crecs))
        for args in (("paf2maf", paf, "-g", t_fa, "-q", q_fa), ("chain2maf", ch, "-g", ct_fa, "-q", cq_fa)):
            for env in ({}, k32.HOST_WRITER):
                rc, out, err = k32.run(cli, "--gpus", "2", *args, "-o", str(tmp_path / "g.maf"), "-r", env=env)
                assert rc == 1 and out == b"" and "only 1 device(s) visible" in err, (args, rc, out, err)
