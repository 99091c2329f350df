"""`chunk` on the CPU: the `wgatools` host code linked against the emulator build of K20 (tests/emu/wgatools_emu), and the
C-ABI entry on the emulator build.  Same cases as test_gpu_maf_chunk.py."""
import os

import pytest

from wgatools_amd import build
import maf_chunk_cases as mc


@pytest.fixture(scope="module")
def cli():
    return build.build_cli_emu()


def test_chunk_fixture_l300(cli):
    mc.check_fixture(cli)


def test_chunk_random_files_and_lengths(cli, tmp_path):
    mc.check_random_files(cli, tmp_path)


def test_chunk_readers_pieces_windows(cli, tmp_path):
    mc.check_readers_pieces_windows(cli, tmp_path)


def test_chunk_empty_inputs(cli, tmp_path):
    mc.check_empty_inputs(cli, tmp_path)


def test_chunk_argument_and_file_errors(cli, tmp_path):
    mc.check_errors(cli, tmp_path)


def test_chunk_streamed_errors(cli, tmp_path):
    mc.check_stream_errors(cli, tmp_path)


def test_chunk_non_ascii_rows_on_the_host(cli, tmp_path):
    """non-ASCII rows go to the host reader: sizes count characters, a cut inside a character panics"""
    path = str(tmp_path / "u.maf")
    open(path, "wb").write("##maf\na score=1\ns a 5 3 + 90 AéC-G\ns b 7 4 - 80 ACGTTA\n\n".encode())
    rc, out, err = mc.run(cli, "chunk", path, "-l", "3")
    assert rc == 0, err
    assert out == ("#maf version=1.6 split_length=3\na score=255\ns\ta\t5\t2\t+\t90\tAé\ns\tb\t7\t3\t-\t80\tACG\n\n"
                   "a score=255\ns\ta\t7\t2\t+\t90\tC-G\ns\tb\t10\t3\t-\t80\tTTA\n\n").encode()
    rc, out, err = mc.run(cli, "chunk", path, "-l", "2")
    assert rc == 1 and "char boundary" in err
    assert out == b"#maf version=1.6 split_length=2\n"


def test_chunk_gpus_on_emulated_devices(cli, tmp_path):
    os.environ["WGA_EMU_DEVICES"] = "3"
    try:
        mc.check_gpus(cli, tmp_path)
    finally:
        os.environ.pop("WGA_EMU_DEVICES", None)


@pytest.fixture(scope="module")
def eng(emu):
    return emu


def test_chunk_abi_windows(eng):
    mc.check_abi_shapes(eng)


def test_chunk_abi_long_rows(eng):
    mc.check_abi_long_rows(eng)


def test_chunk_abi_record_ends_at_tile_edge(eng):
    mc.check_abi_record_ends_at_tile_edge(eng)


def test_chunk_abi_fields_straddle_tile_edge(eng):
    mc.check_abi_fields_straddle_tile_edge(eng)


def test_chunk_abi_many_lines_per_tile(eng):
    mc.check_abi_many_lines_per_tile(eng)
