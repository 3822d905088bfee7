"""GPU: harmony voices — knnsvc_harmony_f0_seg / ops.harmony_f0_seg, knnsvc_mix_waves / ops.mix_waves, and ``harmony`` through
match_features[_many|_blend], serving.BatchConverter (stems, both match routes, a blend, target_duration), special_match and
serving.RequestQueue — against the numpy restatement of the specification in tests/harmony_oracle.py.  Tolerances and their reasons
are in tests/harmony_child.py; tests/test_harmony_cpu.py shows without a GPU that no kernel case stands closer than 1e-6 semitone
to a note decision going the other way, so notes and D are compared exactly.

All GPU work runs in ONE fresh child interpreter (tests/harmony_child.py) that writes a report; the tests only read it, and nothing
here may touch the GPU in the pytest process.  Every test fails without the feature: the names do not exist.

Kernel cases:
  edges       tune_oracle's table (runs of 1, 2, H, H+1, 2H+1, 2H+2 and 40 frames; NaN, +inf and a negative frame; an off segment
              between on ones; adjacent pitched segment ends; masks with d = 1, 5, 6, 7, 12; three tuning frequencies) with a part per
              segment and a segment whose steps are 0: the oracle, guards around f0, notes and workspace, a misaligned input, each
              segment alone and a second call bit-identical
  steps       a stepwise melody x masks d = 1, 5, 7, 12 x steps {+-1, +-2, +-d, +-24} x a {1, 0.39, 0.1}: 96 segments of 954 frames
              (two library calls); degree moves that cross the octave both ways
  one-run     one run of 1500 frames (the sequential lane at the workload's length)
  low         a melody below 8.18 Hz: negative notes, floor division and non-negative remainder
  identities  chromatic = (float)exp(l + steps * S); steps = +-d = an octave, D = +-12: no oracle f0 involved
  seventy     mixed on / off / scales in one ops call (two library calls) == each segment alone; all off: the input object
  mix         1, 3, 1023 and 64 001 samples, 1 and 4 voices, misaligned pointers, a zero-gain voice of NaN, in place: bit-equal to numpy
Product cases (seeded small models, sources written 35 cents sharp): see the test names."""
import pytest
import torch

from tests.gpu_child import check, report_fixture

pytestmark = pytest.mark.gpu
CHILD_TIMEOUT_S = 240        # the GPU work takes seconds, the oracle (a Python loop per frame, the notes of a source computed once
                             # per mask) a few more; the rest is for a cold torch import
report = report_fixture("harmony_child.py", "harmony", CHILD_TIMEOUT_S)


def test_edges_equal_the_oracle_and_nothing_outside_the_table_is_written(report):
    check(report, "kernel/edges/equals-the-oracle", 1)
    check(report, "kernel/edges/guards-untouched", 1)
    check(report, "kernel/edges/off-segments-keep-their-bits", 1)


def test_each_segment_alone_and_a_second_call_are_bit_identical(report):
    check(report, "kernel/edges/each-segment-alone-is-bit-identical", 1)
    check(report, "kernel/edges/second-call-is-bit-identical", 1)


@pytest.mark.parametrize("case", ["steps", "one-run", "low"])
def test_every_mask_step_and_glide_equals_the_oracle_with_notes_and_intervals_exact(report, case):
    check(report, f"kernel/{case}/equals-the-oracle", 1)
    print("largest relative error against the oracle:", report["kernel/largest-oracle-error"]["detail"])


@pytest.mark.parametrize("case", ["steps", "one-run", "low"])
def test_the_chromatic_mask_is_a_parallel_part_and_d_steps_are_an_octave(report, case):
    check(report, f"kernel/{case}/chromatic-is-a-parallel-part", 1)
    check(report, f"kernel/{case}/d-steps-are-an-octave", 1)


def test_largest_oracle_error_is_within_the_bound(report):
    check(report, "kernel/largest-oracle-error", 1)
    check(report, "product/largest-oracle-error", 1)


def test_seventy_segments_in_one_call_equal_each_alone_bit_for_bit(report):
    check(report, "kernel/seventy-segments-equal-each-alone", 1)
    check(report, "kernel/all-off-chunk-is-copied", 1)
    check(report, "kernel/all-off-returns-the-input-object", 1)


def test_ops_refuse_bad_arguments(report):
    check(report, "kernel/ops-refuses", 1)
    check(report, "mix/ops-refuses", 1)
    check(report, "kernel/ran", 1)


@pytest.mark.parametrize("n", [1, 3, 1023, 64001])
def test_mix_waves_is_bit_equal_to_numpy_fp64(report, n):
    check(report, f"mix/{n}-samples", 1)
    check(report, "mix/ran", 1)


def test_defaults_reproduce_the_call_without_the_argument_bit_for_bit(report):
    check(report, "product/defaults-are-bit-identical", 1)


def test_the_lead_stem_is_the_conversion_without_harmony_and_the_mix_is_numpys(report):
    check(report, "product/stems/", exactly=4)
    check(report, "product/special-match-goes-through-the-converter", 1)


@pytest.mark.parametrize("case", ["none", "median", "tune", "blend", "target-duration"])
def test_a_parts_f0_equals_the_oracle_on_the_leads_and_its_features_are_the_leads(report, case):
    check(report, f"product/match/{case}/", at_least=2 if case != "blend" else 1)


@pytest.mark.parametrize("route", ["lanes", "segmented"])
def test_a_mixed_batch_equals_the_single_conversions(report, route):
    check(report, "product/converter/harmony-changes-the-output", 1)
    check(report, f"product/converter/{route}-batch-equals-single", 1)
    check(report, "product/converter/blend", 1)


def test_one_encoder_pass_and_one_search_per_source_and_voice_however_many_parts(report):
    check(report, "product/one-encoder-pass-and-one-search-per-source-and-voice", 1)


def test_requests_with_different_harmonies_share_a_batch_and_a_bad_one_fails_alone(report):
    check(report, "product/queue", 1)


def test_bad_values_are_refused_before_a_file_is_read(report):
    check(report, "product/refusals", 1)
    check(report, "product/ran", 1)


def test_parent_process_left_the_gpu_alone(report):
    assert not torch.cuda.is_initialized()
