"""GPU: topk — 1 to 8 neighbours per frame through the match stage (knnsvc_concat_reselect_seg_k, knnsvc_smooth_weights_seg_k,
knnsvc_weighted_gather's mean_mode, matching.match_features_many(topk=), serving.BatchConverter(topk=), special_match(use_topk=))
against the CPU oracle, which takes k from idx.shape[1], and against fp64 sums.

All GPU work runs in ONE fresh child interpreter (tests/topk_child.py) that writes a report; the tests only read it.  This module
sorts in front of test_gpu_dist2, which must find the interpreter without an initialised GPU, so nothing here may touch the GPU
in the pytest process.

Cases (the smallest shapes that reach every boundary; the bars and their CPU-checked preconditions are in topk_child.py):
  walk            k in {1, 2, 3, 5, 6, 7, 8}, both variants, (1, 40, 64), (2, 40, 256), (3, 9, 768: the clamp, repeated candidates),
                  (64, 48, 1024: the LDS limit at k = 8), (130, 4000, 512): selected sets equal on every frame, on the long pool
                  also the order; one segmented call over [1, 2, 3, 64] at k = 8, bit-identical to the single calls.
  walk-k4         k = 4 past dim 1024, where the default k leaves the pipelined walk for the K kernel: (3, 9, 1280) and
                  (130, 4000, 1280), both variants, judged like the other k.
  walk-generic4   KNNSVC_MATCH_GENERIC_K=1 on fixture g4_select, exact rows.
  smooth          k in {1, 2, 3, 5, 8} on two pools (scale 1000 / 0.1) within 4e-4 of the oracle and the same iteration count;
                  row_scale at k = 5.
  smooth-k4       k = 4 at 1537 rows (the first length past the register loops) on the dim-64 pool, same bar.
  smooth-seg      max_iter 300, segments [1, 2, 2304, 2305] at k = 8 and [1, 2, 37, 6144, 6145] at k = 3 (LDS | global
                  exchange), bit-identical to the single calls.
  smooth-generic4 the knob on fixture g5_smooth, 4e-4 and the fixture's iteration counts.
  gather          k in {3, 5, 6, 7}, both modes, within k 2^-24 max|x| of the fp64 mean; k = 4: both modes and the parent's
                  expression bit-identical.
  chain           match_features_many(topk = 1, 3, 8) on three items (2 / 31 / 150 frames), mix / post_opt_0.2 and
                  wavlm_only / no_post_opt; topk=4 is topk=None and many is single (k = 8), bit for bit.
  product         tiny models: BatchConverter(topk=8) lanes == segmented, != default, finite; special_match ignores topk
                  without use_topk, honours it with, and use_topk with topk=4 is the default, bit for bit."""
import pytest
import torch

from tests.gpu_child import check, report_fixture

pytestmark = pytest.mark.gpu
CHILD_TIMEOUT_S = 600        # a few seconds of GPU work per case; most of the time is the CPU oracle's frame-by-frame walks
report = report_fixture("topk_child.py", "topk", CHILD_TIMEOUT_S, stdout_tail=20000)


def test_walk_for_every_k_equals_the_oracle(report):
    check(report, "walk/", exactly=7 * 5 * 2 + 1)


def test_generic_walk_at_k4_equals_the_oracle(report):
    check(report, "walk-k4/", exactly=2 * 2)


def test_walk_segments_equal_single_sequences_at_k8(report):
    check(report, "walk-seg/", exactly=2)


def test_generic_walk_at_k4_matches_the_reference_fixture(report):
    check(report, "walk-generic4/", exactly=2 + 1)


def test_smooth_weights_for_every_k_equal_the_oracle(report):
    check(report, "smooth/", exactly=2 * 5 + 1 + 1)


def test_long_smooth_weights_at_k4_equal_the_oracle(report):
    check(report, "smooth-k4/", exactly=1 + 1)


def test_smooth_weights_segments_equal_single_sequences(report):
    check(report, "smooth-seg/", exactly=2 + 1)


def test_generic_smooth_weights_at_k4_match_the_reference_fixture(report):
    check(report, "smooth-generic4/", exactly=2 + 1)


def test_uniform_gather_both_modes(report):
    check(report, "gather/", exactly=4 * 2 + 1 + 1)


def test_match_features_many_with_topk(report):
    check(report, "chain/", exactly=2 * (3 * 3 + 2) + 1)


def test_product_entry_points_honour_topk(report):
    check(report, "product/", exactly=6 + 1)


def test_parent_process_left_the_gpu_alone(report):
    assert not torch.cuda.is_initialized()
