"""K19 (wga_maf_call_vcf) on the CPU: the emulator build of the kernel against the oracle, through the C-ABI.  Same cases as
test_gpu_maf_call.py (maf_call_cases.py), the random battery smaller, plus one long block."""
import pytest

import maf_call_cases as mc


@pytest.fixture(scope="module")
def eng(emu):
    return emu


IDS = ["%s%s-l%d-c%d" % ("s" if p[0] else "", "i" if p[1] else "", p[2], p[3]) for p in mc.PARAMS]


@pytest.mark.parametrize("ps", mc.PARAMS, ids=IDS)
def test_k19_step_and_carry_edges(eng, ps):
    mc.check_group(eng, mc.edge_blocks(), ps, "edges", thin=True)


@pytest.mark.parametrize("ps", mc.PARAMS, ids=IDS)
def test_k19_chunk_cuts(eng, ps):
    mc.check_group(eng, mc.cut_blocks(), ps, "cuts")


@pytest.mark.parametrize("ps", mc.PARAMS, ids=IDS)
def test_k19_degenerate_blocks(eng, ps):
    mc.check_group(eng, mc.degenerate_blocks(), ps, "degenerate")


@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 9])
def test_k19_block_counts(eng, n):
    """four waves a workgroup: the last workgroup's waves without a block leave at once"""
    mc.check_block_counts(eng, n)


@pytest.mark.parametrize("ps", mc.PARAMS, ids=IDS)
def test_k19_text_paths(eng, ps):
    mc.check_group(eng, mc.text_blocks(), ps, "text", thin=True)


def test_k19_steps_of_8192_and_8193_bytes(eng):
    mc.check_sized_steps(eng)


@pytest.mark.parametrize("case", mc.bad_base_cases(), ids=lambda c: c[0].replace(" ", "_"))
def test_k19_bad_base(eng, case):
    mc.check_bad_base_case(eng, case)


def test_k19_two_bad_blocks_in_one_call(eng):
    mc.check_two_bad_blocks(eng)


def test_k19_random_battery(eng):
    tot, multi, nbad, late = mc.check_random_battery(eng, range(100, 115))
    print("blocks %d, with a chunk of more than one step %d, bad %d, bad behind the first step %d" % (tot, multi, nbad, late))
    mc.assert_battery_shares(tot, multi, nbad, late)


@pytest.mark.parametrize("chunk", [mc.BIG, 10 ** 4, 333])
def test_k19_one_long_block(eng, chunk):
    """10^6 columns (some 70 000 runs: 1 100 steps in one chunk at the default size); 3 x 10^5 at -c 333, where the emulator's
    time goes by the chunk (900 of them)"""
    mc.check_long_block(eng, 10 ** 6 if chunk >= 10 ** 4 else 3 * 10 ** 5, chunk, pin=chunk >= 10 ** 4)
