"""GPU: pitch control — knnsvc_shift_f0_seg_mode, ops.shift_f0_seg(modes=, transposes=), and f0_shift / transpose through
match_at_inference_time, special_match, serving.BatchConverter and serving.RequestQueue — against the numpy restatement of the
specification in tests/pitch_oracle.py.  Tolerances and their reasons are in tests/pitch_child.py; tests/test_pitch_cpu.py shows
without a GPU that no f0 case stands closer than 0.1 to a rounding tie, so an ulp in a median cannot flip an interval.

All GPU work runs in ONE fresh child interpreter (tests/pitch_child.py) that writes a report; the tests only read it.  This module
sorts in front of test_gpu_dist2, which must find the interpreter without an initialised GPU, so nothing here may touch the GPU in
the pytest process.

Kernel cases (a few hundred to two thousand frames each):
  median-t0              a stacked table (three melodies, an all-unvoiced segment, a segment with one voiced frame, two 1-frame
                         segments) through the new entry with median / 0 == the old entry, bit for bit; the entries share one
                         kernel, so the table is also held against the oracle and against each segment alone (knnsvc_shift_f0)
  up / down / near       every mode x transpose {0, +3, -12, 0.5}: one call per case, the source stacked sixteen times
  seventy-segments       mixed modes and transposes in one ops call (two library calls) == each segment alone, bit for bit
  unvoiced-pool          `none` gives finite output and never reads the NaN median; `median` gives NaN on voiced frames
Product cases (seeded small models): defaults bit-identical to the call without the arguments (fails without the feature: the
arguments do not exist), semitone against the oracle, none + 12 doubles f0, a mixed batch of four on both match routes == the
four single conversions, two requests with different transposes in one queue batch, refusals before a file is read."""
import pytest
import torch

from tests.gpu_child import check, report_fixture

pytestmark = pytest.mark.gpu
CHILD_TIMEOUT_S = 180        # the GPU work takes seconds; the rest is for a cold torch import
report = report_fixture("pitch_child.py", "pitch", CHILD_TIMEOUT_S)


def test_median_without_transpose_through_the_new_entry_is_the_old_entry_bit_for_bit(report):
    check(report, "kernel/median-t0-is-the-old-entry", 1)
    check(report, "kernel/median-t0-reports-the-interval", 1)
    # the entries share one kernel: the same table against the oracle, and each segment alone through knnsvc_shift_f0
    check(report, "kernel/median-t0-equals-the-oracle-and-each-segment-alone", 1)


@pytest.mark.parametrize("case", ["up", "down", "near"])
def test_every_mode_and_transpose_equals_the_oracle(report, case):
    check(report, f"kernel/{case}/precondition", 1)
    check(report, f"kernel/{case}/mode", 16)
    print("largest relative error against the oracle:", report["kernel/largest-oracle-error"]["detail"])


def test_largest_oracle_error_is_within_the_bound(report):
    check(report, "kernel/largest-oracle-error", 1)


def test_seventy_segments_in_one_call_equal_each_alone_bit_for_bit(report):
    check(report, "kernel/seventy-segments-equal-each-alone", 1)


def test_none_never_reads_the_medians_and_median_propagates_nan(report):
    check(report, "kernel/unvoiced-pool", 1)
    check(report, "kernel/ops-refuses", 1)
    check(report, "kernel/ran", 1)


def test_defaults_reproduce_the_call_without_the_arguments_bit_for_bit(report):
    check(report, "product/defaults-are-bit-identical", 1)


def test_semitone_mode_equals_the_oracle_and_changes_the_waveform(report):
    check(report, "product/precondition", 1)
    check(report, "product/semitone", 2)


def test_transpose_12_without_a_shift_doubles_every_voiced_f0(report):
    check(report, "product/none-plus-12-doubles", 1)


@pytest.mark.parametrize("route", ["lanes", "segmented"])
def test_a_batch_of_four_settings_equals_the_four_single_conversions(report, route):
    check(report, "product/converter/settings-change-the-output", 1)
    check(report, f"product/converter/{route}-batch-equals-single", 1)


def test_two_requests_with_different_transposes_share_a_batch(report):
    check(report, "product/queue", 1)


def test_bad_values_are_refused_before_a_file_is_read(report):
    check(report, "product/refusals", 1)
    check(report, "product/largest-oracle-error", 1)
    check(report, "product/ran", 1)


def test_parent_process_left_the_gpu_alone(report):
    assert not torch.cuda.is_initialized()
