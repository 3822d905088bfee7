"""GPU: voice blending — knnsvc_blend_seg, knnsvc_shift_f0_seg_blend, ops.blend_seg / shift_f0_seg_blend,
matching.match_features_blend, and the weights through serving.BatchConverter, serving.RequestQueue, special_match and
many_to_one — against the numpy restatement of the specification in tests/blend_oracle.py.  What is asked and why is in
tests/blend_child.py; tests/test_blend_cpu.py holds what needs no GPU.  Every comparison is bit equality.

All GPU work runs in ONE fresh child interpreter (tests/blend_child.py) that writes a report; the tests only read it.  This
module sorts in front of test_gpu_dist2, which must find the interpreter without an initialised GPU, so nothing here may touch
the GPU in the pytest process.

Kernel cases (features bit-identical to the oracle):
  dims              T = 300 at V = 2, 3, 4 and dim 1024 (vector path), 49 (the harmonics' width) and 7 (scalar path), each also
                    with one voice's pointer one float off a 16-byte boundary
  edges             one call stacking segments of 1, 2, 5 and 300 rows with a vector each: a one-hot vector (the segment equals
                    its input bit for bit), a zero weight on a voice that is NaN everywhere; every segment alone == its slice
  seventy-segments  3..40 rows each, one ops call (two library calls) == each segment alone
  canary            64 guard rows of a sentinel around the output stay untouched, dim 1024 and 7
  shift             ops.shift_f0_seg_blend in all four modes with transposes on a melody with rests and three voices' medians ==
                    the existing ops.shift_f0_seg with ``pmed`` = the oracle's blended fp32 median, bit for bit; a one-hot vector
                    == the shift towards that voice; a NaN median is ignored under weight 0 and propagates above it
Product cases (seeded small models, synthetic clips): [1, 0] / [0, 1] on (A, B) and [.5, .5] on (A, A) bit-identical to the
single-target conversions, (A, B, [.3, .7]) == (B, A, [.7, .3]), a single TargetVoice unchanged, [.5, .5] on (A, B) == the chain
by hand and different from both single conversions, a batch of four with per-source weights on both match routes == the single
conversions, queue requests with different weights in one batch and a bad vector failing alone, the blend together with
target_duration, the written files' names.  They fail without the feature: the arguments and entries do not exist."""
import pytest
import torch

from tests.gpu_child import check, report_fixture

pytestmark = pytest.mark.gpu
CHILD_TIMEOUT_S = 240        # the GPU work takes seconds; the rest is for a cold torch import
report = report_fixture("blend_child.py", "blend", CHILD_TIMEOUT_S)


@pytest.mark.parametrize("V", [2, 3, 4])
@pytest.mark.parametrize("dim", [1024, 49, 7])
def test_vector_scalar_and_unaligned_paths_are_bit_identical_to_the_oracle(report, dim, V):
    check(report, f"kernel/dims/{dim}/v{V}", 2)


def test_edge_segments_in_one_call_equal_the_oracle_and_each_segment_alone(report):
    check(report, "kernel/edges/bit-identical", 1)
    check(report, "kernel/edges/each-segment-alone", 1)


def test_a_one_hot_segment_is_its_input_and_a_zero_weight_voice_is_not_read(report):
    check(report, "kernel/edges/one-hot-segment-is-its-input", 1)
    check(report, "kernel/edges/single-term-copies-bit-for-bit", 1)
    check(report, "kernel/edges/a-positive-weight-lets-nan-through", 1)


def test_seventy_segments_in_one_call_equal_each_alone_bit_for_bit(report):
    check(report, "kernel/seventy-segments-equal-each-alone", 1)


@pytest.mark.parametrize("dim", [1024, 7])
def test_guard_rows_around_the_output_are_untouched(report, dim):
    check(report, f"kernel/canary/{dim}", 1)


def test_ops_refuses_bad_tables_and_the_kernel_cases_ran(report):
    check(report, "kernel/ops-refuses", 1)
    check(report, "kernel/ran", 1)
    print("kernel time:", report["kernel/timing-1500x1024-v2"]["detail"])


def test_blended_shift_equals_the_existing_shift_towards_the_blended_median(report):
    check(report, "shift/equals-the-existing-shift-towards-the-blended-median", 1)
    check(report, "shift/default-tables-are-the-median-shift", 1)
    check(report, "shift/seventy-segments-equal-each-alone", 1)


def test_one_hot_shift_and_nan_medians(report):
    check(report, "shift/one-hot-is-the-shift-towards-that-voice", 1)
    check(report, "shift/nan-median-ignored-at-weight-zero-propagates-above", 1)
    check(report, "shift/ran", 1)


def test_a_single_target_voice_without_blend_is_unchanged(report):
    check(report, "product/single-voice-is-unchanged", 1)


@pytest.mark.parametrize("case", ["one-zero-is-towards-A", "zero-one-is-towards-B", "half-half-of-A-and-A-is-A", "swapping-voices-and-weights"])
def test_identities_are_bit_identical_to_the_single_target_conversion(report, case):
    check(report, f"product/identity/{case}", 1)


def test_half_half_equals_the_chain_by_hand_and_differs_from_both_voices(report):
    check(report, "product/chain-by-hand", 1)
    check(report, "product/half-half-differs-from-both", 1)


@pytest.mark.parametrize("route", ["lanes", "segmented"])
def test_a_batch_with_per_source_weights_equals_the_single_conversions(report, route):
    check(report, "product/converter/single-conversions", 1)
    check(report, f"product/converter/{route}-batch-equals-single", 1)


def test_requests_with_different_weights_share_a_batch_and_a_bad_vector_fails_alone(report):
    check(report, "product/queue/", 1)


def test_the_blend_works_together_with_target_duration(report):
    check(report, "product/with-target-duration", 1)


def test_the_written_files_are_named_after_the_voices(report):
    check(report, "product/files", 1)
    check(report, "product/ran", 1)


def test_parent_process_left_the_gpu_alone(report):
    assert not torch.cuda.is_initialized()
