"""GPU: pitch correction — knnsvc_tune_f0_seg, ops.tune_f0_seg, and ``tune`` through match_at_inference_time, special_match,
match_features[_many|_blend], serving.BatchConverter and serving.RequestQueue — against the numpy restatement of the specification
in tests/tune_oracle.py.  Tolerances and their reasons are in tests/tune_child.py; tests/test_tune_cpu.py shows without a GPU that
no kernel case stands closer than 1e-6 semitone to a note decision going the other way, so notes are compared exactly.

All GPU work runs in ONE fresh child interpreter (tests/tune_child.py) that writes a report; the tests only read it.  This module
runs in front of test_gpu_dist2, which must find the interpreter without an initialised GPU, so nothing here may touch the GPU in
the pytest process.

Kernel cases (a few hundred to two thousand frames per segment):
  edges                  one stacked table of hand-made segments (runs of 1, 2, H, H+1, 2H+1, 2H+2 and 40 frames; a run at frame 0
                         and one at the last frame; a segment ending pitched before one starting pitched 3 semitones away; an
                         all-unvoiced segment; 1-frame segments; NaN, +inf and a negative frame inside a melody; an off segment
                         between on segments; a different mask, strength, retune and tuning frequency per segment): equal to the
                         oracle, guards untouched around f0, notes and workspace, misaligned input, each segment alone and a
                         second call bit-identical
  up / down / near       raw and median-shifted, {chromatic, C:major, G:major, a custom pattern} x {(1, 0), (1, 80), (0.6, 200)}
  steps, one-run         long runs: 36 notes 35 cents sharp; one run of 1500 frames (the sequential lane at the workload's length)
  hard-snap              strength 1, retune 0: every pitched output on tuning_hz * 2^((note - 69) / 12), no oracle f0 involved
  seventy-segments       mixed on / off / scales in one ops call (two library calls) == each segment alone; all off: the input object
Product cases (seeded small models, sources written 35 cents sharp): defaults bit-identical to the call without the argument
(fails without the feature: the argument does not exist), f0 against the oracle under f0_shift none / median / a blend /
target_duration, a mixed batch of four on both match routes == the four single conversions, requests with different scales in
one queue batch, refusals before a file is read."""
import pytest
import torch

from tests.gpu_child import check, report_fixture

pytestmark = pytest.mark.gpu
CHILD_TIMEOUT_S = 240        # the GPU work takes seconds, the oracle (a Python loop per frame over some 90 000 frames) a few more;
                             # the rest is for a cold torch import
report = report_fixture("tune_child.py", "tune", CHILD_TIMEOUT_S)


def test_edges_equal_the_oracle_and_nothing_outside_the_table_is_written(report):
    check(report, "kernel/edges/equals-the-oracle", 1)
    check(report, "kernel/edges/guards-untouched", 1)
    check(report, "kernel/edges/off-segment-keeps-its-bits", 1)


def test_each_segment_alone_and_a_second_call_are_bit_identical(report):
    check(report, "kernel/edges/each-segment-alone-is-bit-identical", 1)
    check(report, "kernel/edges/second-call-is-bit-identical", 1)


@pytest.mark.parametrize("case", ["up", "up-shifted", "down", "down-shifted", "near", "near-shifted", "steps", "one-run"])
def test_every_mask_and_setting_equals_the_oracle(report, case):
    check(report, f"kernel/{case}/equals-the-oracle", 1)
    print("largest relative error against the oracle:", report["kernel/largest-oracle-error"]["detail"])


@pytest.mark.parametrize("case", ["up", "up-shifted", "down", "down-shifted", "near", "near-shifted", "steps", "one-run"])
def test_a_hard_snap_lands_on_the_grid_without_asking_the_oracle(report, case):
    check(report, f"kernel/{case}/hard-snap-lands-on-the-grid", 1)


def test_largest_oracle_error_is_within_the_bound(report):
    check(report, "kernel/largest-oracle-error", 1)


def test_seventy_segments_in_one_call_equal_each_alone_bit_for_bit(report):
    check(report, "kernel/seventy-segments-equal-each-alone", 1)
    check(report, "kernel/all-off-chunk-is-copied", 1)
    check(report, "kernel/all-off-returns-the-input-object", 1)


def test_ops_refuses_bad_arguments(report):
    check(report, "kernel/ops-refuses", 1)
    check(report, "kernel/ran", 1)


def test_defaults_reproduce_the_call_without_the_argument_bit_for_bit(report):
    check(report, "product/defaults-are-bit-identical", 1)


def test_a_key_without_a_shift_equals_the_oracle_and_changes_the_waveform(report):
    check(report, "product/none-with-a-key/", exactly=2)


def test_a_key_behind_the_median_shift_equals_the_oracle_and_the_debug_dict_carries_the_notes(report):
    check(report, "product/median-with-a-key/f0-equals-the-oracle", 1)
    check(report, "product/debug-dict", 1)


@pytest.mark.parametrize("route", ["lanes", "segmented"])
def test_a_batch_of_four_settings_equals_the_four_single_conversions(report, route):
    check(report, "product/converter/settings-change-the-output", 1)
    check(report, f"product/converter/{route}-batch-equals-single", 1)


def test_a_blend_with_a_key_equals_the_oracle_on_the_blends_untuned_f0(report):
    check(report, "product/blend/", exactly=2)


def test_target_duration_with_a_key_equals_the_oracle_on_the_retimed_f0(report):
    check(report, "product/with-target-duration/", exactly=2)


def test_requests_with_different_scales_share_a_batch_and_a_bad_one_fails_alone(report):
    check(report, "product/queue", 1)


def test_bad_values_are_refused_before_a_file_is_read(report):
    check(report, "product/refusals", 1)
    check(report, "product/largest-oracle-error", 1)
    check(report, "product/ran", 1)


def test_parent_process_left_the_gpu_alone(report):
    assert not torch.cuda.is_initialized()
