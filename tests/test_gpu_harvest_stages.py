"""GPU: Harvest f0 (csrc/harvest.hip) stage by stage against oracle/f0_ref.py — decimation, mean, channel table, band-pass bank,
event lists, raw channel f0, candidates, refinement, reliability, base / step 1 / step 2, extension, merge, gap bridging, smoothing,
sampling and status — each stage of the device against the oracle's stage applied to the device's own previous output (teacher
forcing), and the whole track against the oracle run from the waveform.  The cases reach what no other fixture does: the minimum
length, ylen either side of the bank's 1024-sample tile, L + 18 either side of the IIR's 64-sample chunk, dozens of short sections,
every branch of the merge, nk == 0, both ends of the smoother cut and uncut, a track wholly under zero_below, a section dropped by
the 2200 / mean rule, other floors / ceilings / frame periods.  The workspace is read back through
knnsvc_debug_f0_harvest_layout; poisoning (0x00 / 0xFF), padding gaps, guard bytes, high-water marks and the C entry's refusals
are checked too.  Rules, cases and references: tests/harvest_child.py, tests/harvest_oracle.py; tests/test_harvest_cpu.py checks
both without a GPU.

Value stages, worst error over all cases measured on the MI355X (max |device - reference| / max |reference|) and the bar (eight
times that, rounded up to a power of ten; none may exceed 1e-9) — see profiles/harvest_errors.txt:
    decimate           6.5e-16 (low-70)            bar 1e-14
    bank               3.0e-15 (low-70)            bar 1e-13
    refine/pitch       1.1e-14 (merge)             bar 1e-13
    refine/deviation   3.1e-11 (params/100-500-1)  bar 1e-9    the FFT reference's error at the weakest harmonic's bin
    smooth             5.6e-15 (dense)             bar 1e-13
Decision stages: every integer and zero pattern equal on every case, no element excluded anywhere, values within 6.9e-16 (bar 2^-40).

All GPU work runs in ONE fresh child interpreter (tests/harvest_child.py) that writes a report; the tests only read it.  This
module runs in front of test_gpu_dist2, which must find the interpreter without an initialised GPU, so nothing here may touch the
GPU in the pytest process."""
import pytest
import torch

from tests import harvest_oracle as O
from tests.gpu_child import check, report_fixture

pytestmark = pytest.mark.gpu
CHILD_TIMEOUT_S = 70         # the child's wall time on the MI355X machine, 12.3 s alone and 14.4 s inside the whole suite (most of it
                             # the fp64 references on the CPU), times five
report = report_fixture("harvest_child.py", "harvest", CHILD_TIMEOUT_S, stdout_tail=60000)

STAGES = ("decimate", "mean", "centre", "channels", "bank", "events", "raw", "candidates", "refine/pitch", "refine/deviation",
          "refine/gates", "reliable", "base", "step1", "step2", "extend", "merge", "bridge", "smooth", "sample", "track")
# family -> the number of entries the child writes for it
ENTRIES = {"stage/": len(O.CASES) * len(STAGES), "workspace/": 4 * len(O.WORKSPACE_CASES), "args/": 10 + 1, "summary/": 18}


@pytest.mark.parametrize("case", sorted(O.CASES))
def test_every_stage_of_the_case_matches_the_oracle(report, case):
    check(report, f"stage/{case}/", exactly=len(STAGES))            # no case name is the prefix of another
    for stage in STAGES:
        print(stage, report[f"stage/{case}/{stage}"]["detail"])


@pytest.mark.parametrize("family", sorted(ENTRIES))
def test_every_check_of_the_family_ran_and_holds(report, family):
    check(report, family, exactly=ENTRIES[family])
    for k in sorted(report):
        if k.startswith(family) and family != "stage/":
            print(k, report[k]["detail"])


def test_both_case_functions_ran_to_their_end(report):
    check(report, "stages/ran", exactly=1)
    check(report, "args/ran", exactly=1)


def test_parent_process_left_the_gpu_alone(report):
    assert not torch.cuda.is_initialized()
