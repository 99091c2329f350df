"""K16 (wga_paf_call_vcf) on the GPU: the product library against the oracle, through the C-ABI.  The cases of
test_emu_paf_call_vcf.py (paf_call_vcf_cases.py) and a larger random battery."""
import pytest

import paf_call_vcf_cases as pc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng(gpu):
    return gpu


@pytest.mark.parametrize("neg", [False, True], ids=["plus", "minus"])
def test_k16_event_counts(eng, neg):
    pc.check_event_counts(eng, neg)


@pytest.mark.parametrize("kind", ["I", "D", "X1", "X2", "X70"])
def test_k16_rows_at_step_borders(eng, kind):
    pc.check_edges(eng, kind)


@pytest.mark.parametrize("shift", range(16))
@pytest.mark.parametrize("nbytes", [8191, 8192, 8193])
def test_k16_step_of_stage_size(eng, nbytes, shift):
    pc.check_sized_step(eng, nbytes, shift)


def test_k16_text_paths(eng):
    pc.check_text_paths(eng)


@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 9])
def test_k16_record_counts(eng, n):
    pc.check_record_counts(eng, n)


@pytest.mark.parametrize("svlen", pc.SVLENS)
def test_k16_names_and_numbers(eng, svlen):
    pc.check_names_and_numbers(eng, svlen)


@pytest.mark.parametrize("case", pc.error_cases(), ids=lambda c: c[0].replace(" ", "_"))
def test_k16_error(eng, case):
    pc.check_error_case(eng, case)


def test_k16_two_bad_records_in_one_call(eng):
    pc.check_two_bad_records(eng)


@pytest.mark.parametrize("case", pc.ZERO_CASES, ids=lambda c: "%s-%s" % (c[0], "snp" if c[1] else "nosnp"))
def test_k16_zero_length_op_in_front_of_an_indel(eng, case):
    pc.check_zero_length_op(eng, case)


def test_k16_empty_target_on_a_minus_record(eng):
    pc.check_empty_target(eng)


@pytest.mark.parametrize("op", ["D", "I"])
def test_k16_split_indel_error_path(eng, op):
    pc.check_split_indel(eng, op)


def test_k16_random_battery(eng):
    tot, multi, nbad, late = pc.check_random_battery(eng, range(1000, 1060), n_recs=24)
    print("records %d, of more than one step %d, bad %d, bad behind the first step %d" % (tot, multi, nbad, late))
    pc.assert_battery_shares(tot, multi, nbad, late)
