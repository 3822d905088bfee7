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
import json
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD_TIMEOUT_S = 300        # the child takes well under a minute of GPU work plus the imports and the tiny models' graph captures


@pytest.fixture(scope="module")
def report(tmp_path_factory):
    if torch.cuda.is_initialized():
        pytest.skip("ranks are spawned from a process that has not initialised the GPU: run this module first / on its own")
    out = str(tmp_path_factory.mktemp("match_seg") / "report.json")
    try:
        r = subprocess.run([sys.executable, "tests/match_seg_child.py", out], timeout=CHILD_TIMEOUT_S, cwd=ROOT,
                           capture_output=True, text=True)
    except subprocess.TimeoutExpired as e:
        return {"__failed__": f"child timed out after {CHILD_TIMEOUT_S} s\n" + str(e.stderr or "")[-3000:]}
    print(r.stdout[-6000:])
    rep = {}
    if os.path.isfile(out):
        rep = json.load(open(out))
    if r.returncode != 0:
        rep["__failed__"] = f"child exited with {r.returncode}\n" + r.stderr[-3000:]
    return rep


def _check(report, prefix, at_least):
    assert "__failed__" not in report, report["__failed__"]
    mine = {k: v for k, v in report.items() if k.startswith(prefix)}
    assert len(mine) >= at_least, (prefix, sorted(mine))
    bad = {k: v["detail"] for k, v in mine.items() if not v["ok"]}
    assert not bad, bad


def test_walk_segments_equal_single_sequences(report):
    _check(report, "walk/", 2 * 4 * 2 + 1)


def test_walk_segment_output_does_not_depend_on_position(report):
    _check(report, "walk-swapped/", 2 * 4 * 2)


def test_median_and_shift_segments_equal_single_sequences(report):
    _check(report, "median/", 3)
    _check(report, "shift/", 1)


def test_smooth_weights_segments_equal_single_sequences(report):
    _check(report, "smooth/", 2 * 2 * 2 * 3 + 1)


def test_single_smooth_weights_fits_its_own_workspace_size(report):
    _check(report, "single_ws/", 5 * 2 + 1)


def test_wrappers_split_more_than_64_segments(report):
    _check(report, "chunking/", 2)


def test_match_features_many_equals_match_features(report):
    _check(report, "match_many/", 5 + 1)


def test_segmented_product_route_equals_lanes(report):
    _check(report, "product/", 2 * (3 + 1) + 1)


def test_parent_process_left_the_gpu_alone(report):
    assert not torch.cuda.is_initialized()
