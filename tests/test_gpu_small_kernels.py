"""GPU: the small kernels that carry data between the stages — layernorm, wavlm_conv0, wavlm_gate, mask_rows, reflect_pad[_batch],
complex_mag / harmonic_amps / spec_harm, additive_synth, absmax, mean3, axpy, weighted_gather, amp_ratio, round_f16 — each against
a plain reference at the shapes where it takes another branch: dims off the 256-column step, partly filled row groups, row strides
wider than the row with sentinel padding, split (f16x2) outputs and inputs, the multi-span conv0 route, positions that end in
exactly .5, the zero pad bin and both interpolation clamps, launches sized for a bucket with the count on the device, the capped
grids' second pass, column tails, misaligned pointers and NaN.  The comparison rules (bit equality, the bound an existing test has,
or four times the fp32 torch evaluation's own error against fp64) are stated in tests/small_kernels_child.py, the references and
case generators in tests/small_kernels_oracle.py, and tests/test_small_kernels_cpu.py checks both without a GPU.

All GPU work runs in ONE fresh child interpreter (tests/small_kernels_child.py) that writes a report; the tests only read it.  This
module runs in front of test_gpu_dist2, which must find the interpreter without an initialised GPU, so nothing here may touch the
GPU in the pytest process."""
import pytest
import torch

from tests.gpu_child import check, report_fixture

pytestmark = pytest.mark.gpu
CHILD_TIMEOUT_S = 35         # the child's wall time on the MI355X, 4.8 s warm to 6.5 s on a fresh machine (half of it the torch import
                             # and the fp64 references on the CPU), times about five
report = report_fixture("small_kernels_child.py", "small_kernels", CHILD_TIMEOUT_S)

# family -> the number of entries the child writes for it
ENTRIES = {
    "layernorm/": 236, "wavlm_conv0/": 605, "wavlm_gate/": 24, "mask_rows/": 3, "reflect_pad/": 15, "reflect_pad_batch/": 4,
    "complex_mag/": 20, "harmonic_amps/": 150, "spec_harm/": 225, "additive_synth/": 182, "absmax/": 12, "mean3/": 36, "axpy/": 12,
    "weighted_gather/": 108, "amp_ratio/": 36, "round_f16/": 8,
}


@pytest.mark.parametrize("family", sorted(ENTRIES))
def test_every_check_of_the_family_ran_and_holds(report, family):
    check(report, family, at_least=ENTRIES[family])
    for k in sorted(report):
        if k.startswith("summary/" + family):
            print(k, report[k]["detail"])


def test_every_case_function_ran_to_its_end(report):
    check(report, "summary/", at_least=len(ENTRIES))
    for case in ("layernorm", "wavlm_conv0", "wavlm_gate", "mask_rows", "reflect_pad", "reflect_pad_batch", "side_feature",
                 "additive_synth", "absmax", "mean3_axpy", "match_helper"):
        check(report, f"{case}_cases/ran", exactly=1)


def test_parent_process_left_the_gpu_alone(report):
    assert not torch.cuda.is_initialized()
