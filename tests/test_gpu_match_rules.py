"""The match stage's rules and optimiser routes against fp64 and the CPU oracle.  Everything that touches the GPU runs in ONE child
interpreter (tests/match_rules_child.py, which says what each family asks); the tests here only read its report.  What makes the
child's inputs fair tests is asserted without a GPU in tests/test_match_rules_cpu.py."""
import pytest
import torch

import match_rules_oracle as R
from tests.gpu_child import check, report_fixture

pytestmark = pytest.mark.gpu
CHILD_TIMEOUT_S = 60         # five times the 12 s the child took on the MI355X, CPU references included (profiles/match_rules_errors.txt)
report = report_fixture("match_rules_child.py", "match_rules", CHILD_TIMEOUT_S, stdout_tail=30000)


def test_every_optimiser_route_after_n_iterations_equals_fp64(report):
    check(report, "smooth/", exactly=len(R.smooth_cases()) + 1)


def test_walk_rules_for_every_k_and_both_kernels_equal_the_oracle(report):
    check(report, "walk/", exactly=2 * len(R.walk_cases()) + 1)


def test_log_f0_median_at_its_edges(report):
    check(report, "median/", exactly=len(R.median_cases()) + 1)


def test_f0_rerank_is_the_stable_argsort_for_every_k(report):
    check(report, "rerank/", exactly=len(R.RERANK_K) * len(R.RERANK_NQ) + 1)


def test_family_sizes():
    assert (len(R.smooth_cases()), len(R.walk_cases()), len(R.median_cases()), len(R.RERANK_K) * len(R.RERANK_NQ)) == (83, 17, 14, 35)


def test_parent_process_left_the_gpu_alone():
    assert not torch.cuda.is_initialized()
