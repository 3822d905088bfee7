"""GPU: the segmented match stage (knnsvc_*_seg, ops.*_seg, matching.match_features_many, the "segmented" route of
serving.BatchConverter) against the single-sequence code it is made of.  Every comparison is EXACT: segment s of a segmented
call is bit-identical to the single-sequence entry point called on that segment's rows alone, so the parity of the single-sequence
entry points with the reference's fixtures (g4, g4c, g5, g5c) carries over without a tolerance.

All GPU work runs in ONE fresh child interpreter (tests/match_seg_child.py) that writes a report; the tests only read it.  This
module sorts in front of test_gpu_dist2, which must find the interpreter without an initialised GPU, so nothing here may touch
the GPU in the pytest process.

Cases (the smallest sizes that reach every kernel variant and boundary):
  walk       segments [1, 2, 3, 5, 64, 257, 1], both variants, pools of 40 (clamp, repeated candidates) and 300 rows, dims 64 /
             1000 / 1024 (pipelined kernel) and 1280 (generic kernel); two segments swapped.
  median     segments [1, 7, 1024, 1025, 3000]: all-unvoiced (NaN median), a single voiced frame, an even voiced count.
  smooth     [1, 2, 37, 512, 513, 1024, 1025, 1536, 1537] (every register variant, the LDS loop) and [4700, 3] (global exchange
             buffer); scale 0.1 on a dim-64 pool, 1000 on a dim-49 pool with ld 64; with and without row_scale; max_iter 300.
  single_ws  knnsvc_smooth_weights (the one-segment case) in a workspace of exactly its own size at a base 4 bytes off alignment, between
             sentinel bytes: [1, 2, 513, 1537, 4609] rows, with and without row_scale, max_iter 50.
  chunking   70 segments through the wrappers (two library calls).
  match_many six items of 1 / 2 / 31 / 150 / 151 / 600 frames, "mix" and "wavlm_only", with and without post_opt, synth_list once.
  product    BatchConverter(match="segmented", match_batch=4) against match="lanes", both generator kinds, three runs; many_to_one
             files under KNNSVC_MATCH=segmented."""
import pytest
import torch

from tests.gpu_child import check, report_fixture

pytestmark = pytest.mark.gpu
CHILD_TIMEOUT_S = 300        # the child takes well under a minute of GPU work plus the imports and the tiny models' graph captures
report = report_fixture("match_seg_child.py", "match_seg", CHILD_TIMEOUT_S, stdout_tail=6000)


def test_walk_segments_equal_single_sequences(report):
    check(report, "walk/", 2 * 4 * 2 + 1)


def test_walk_segment_output_does_not_depend_on_position(report):
    check(report, "walk-swapped/", 2 * 4 * 2)


def test_median_and_shift_segments_equal_single_sequences(report):
    check(report, "median/", 3)
    check(report, "shift/", 1)


def test_smooth_weights_segments_equal_single_sequences(report):
    check(report, "smooth/", 2 * 2 * 2 * 3 + 1)


def test_single_smooth_weights_fits_its_own_workspace_size(report):
    check(report, "single_ws/", 5 * 2 + 1)


def test_wrappers_split_more_than_64_segments(report):
    check(report, "chunking/", 2)


def test_match_features_many_equals_match_features(report):
    check(report, "match_many/", 5 + 1)


def test_segmented_product_route_equals_lanes(report):
    check(report, "product/", 2 * (3 + 1) + 1)


def test_parent_process_left_the_gpu_alone(report):
    assert not torch.cuda.is_initialized()
