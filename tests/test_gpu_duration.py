"""GPU: target_duration — knnsvc_time_scale_seg, ops.time_scale_seg / time_scale, matching.stretch_queries, and the argument
through match_at_inference_time, special_match, serving.BatchConverter and serving.RequestQueue — against the numpy restatement
of the specification in tests/duration_oracle.py.  What is asked and why is in tests/duration_child.py; tests/test_duration_cpu.py
holds the oracle against torch.nn.functional.interpolate without a GPU.

All GPU work runs in ONE fresh child interpreter (tests/duration_child.py) that writes a report; the tests only read it.  This
module sorts in front of test_gpu_dist2, which must find the interpreter without an initialised GPU, so nothing here may touch
the GPU in the pytest process.

Kernel cases (a few hundred to two thousand frames each), features bit-identical to the oracle, f0 pattern equal and voiced
values within 1 fp32 ulp:
  edges             one call stacking T = 1 -> 2, 2 -> 1, 2 -> 8 (s = 4), 8 -> 2 (s = 0.25), 5 with c = 1, 300 with s = 1.37 and
                    0.73, at dim 1024; every segment alone is bit-identical to its slice, the c = 1 segment to its input
  dims              T = 300, s = 1.37 at dim 1024, the small model's width and 7 (scalar path), each also with the feature
                    pointer one float off a 16-byte boundary
  seventy-segments  3..40 rows each, scales in [0.25, 4], one ops call (two library calls) == each segment alone
  f0-edges          a melody with rests, one voiced frame, no voiced frame, a row of ties; features-NULL and f0-NULL forms
  canary            64 guard rows of a sentinel around both outputs stay untouched
Product cases (seeded small models): defaults bit-identical to the call without the argument (fails without the feature: the
argument does not exist), s = 1 bit-identical to the plain conversion, s = 1.25 / 0.8 bit-identical to encode -> ops.time_scale
-> match_features -> Tail by hand with T_out * 320 samples, a batch with [None, shorter, longer, None] on both match routes ==
the four single conversions, requests with different durations in one queue batch and a bad ratio failing alone, the written
file's length and name, refusals before a file is read."""
import pytest
import torch

from tests.gpu_child import check, report_fixture

pytestmark = pytest.mark.gpu
CHILD_TIMEOUT_S = 180        # the GPU work takes seconds; the rest is for a cold torch import
report = report_fixture("duration_child.py", "duration", CHILD_TIMEOUT_S)


def test_edge_segments_in_one_call_equal_the_oracle_and_each_segment_alone(report):
    check(report, "kernel/edges/features-bit-identical", 1)
    check(report, "kernel/edges/f0", 1)
    check(report, "kernel/edges/each-segment-alone", 1)
    check(report, "kernel/edges/scale-one-is-the-input", 1)


@pytest.mark.parametrize("dim", [1024, 128, 7])
def test_vector_scalar_and_unaligned_paths_are_bit_identical_to_the_oracle(report, dim):
    check(report, f"kernel/dims/{dim}", 2)


def test_seventy_segments_in_one_call_equal_each_alone_bit_for_bit(report):
    check(report, "kernel/seventy-segments-equal-each-alone", 1)


def test_f0_edges_in_the_features_null_and_the_f0_null_form(report):
    check(report, "kernel/f0-edges/", 2)
    print("f0 frames that differ from the oracle:", report["kernel/f0-frames-that-differ-from-the-oracle"]["detail"])


@pytest.mark.parametrize("dim", [1024, 7])
def test_guard_rows_around_the_outputs_are_untouched(report, dim):
    check(report, f"kernel/canary/{dim}", 1)


def test_ops_refuses_bad_tables_and_the_kernel_cases_ran(report):
    check(report, "kernel/ops-refuses", 1)
    check(report, "kernel/ran", 1)
    print("kernel time:", report["kernel/timing-1500x1024-s1.25"]["detail"])


def test_defaults_reproduce_the_call_without_the_argument_bit_for_bit(report):
    check(report, "product/defaults-are-bit-identical", 1)


def test_the_sources_own_length_is_the_plain_conversion_bit_for_bit(report):
    check(report, "product/identity", 1)


@pytest.mark.parametrize("tag", ["longer", "shorter"])
def test_the_product_equals_the_chain_by_hand_and_has_the_planned_length(report, tag):
    check(report, f"product/chain/{tag}", 1)


@pytest.mark.parametrize("route", ["lanes", "segmented"])
def test_a_batch_with_mixed_durations_equals_the_single_conversions(report, route):
    check(report, "product/converter/lengths", 1)
    check(report, f"product/converter/{route}-batch-equals-single", 1)


def test_requests_with_different_durations_share_a_batch_and_a_bad_ratio_fails_alone(report):
    check(report, "product/queue/", 2)


def test_the_written_file_has_the_planned_length_under_the_unchanged_name(report):
    check(report, "product/files", 1)


def test_bad_values_are_refused_before_a_file_is_read(report):
    check(report, "product/refusals", 1)
    check(report, "product/ran", 1)


def test_parent_process_left_the_gpu_alone(report):
    assert not torch.cuda.is_initialized()
