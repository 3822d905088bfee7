"""GPU: output loudness (knnsvc_loudness / knnsvc_loudness_gain, ops.loudness / ops.normalize_loudness, the normalize_loudness /
loudness_db switches of special_match, bulk_match, many_to_one and serving.BatchConverter) against the fp64 oracle in
tests/loudness_oracle.py.  Tolerances and their reasons are in tests/loudness_child.py.

All GPU work runs in ONE fresh child interpreter (tests/loudness_child.py) that writes a report; the tests only read it.  This
module sorts in front of test_gpu_dist2, which must find the interpreter without an initialised GPU, so nothing here may touch
the GPU in the pytest process.

Cases (the smallest sizes that reach every path and boundary; C = 64 samples per lane and W = 8192 per workgroup, read from the
library: ops.loudness_layout):
  oracle       16 kHz noise of 0, 1, 6399, 6400 (one block), 7999, 8000 (two), 8001 samples; lengths 6400 + {C-1, C, C+1}, W-1, W,
               W+1 and 3W+C+1 (last chunk short / exact / one over, one and several workgroups); a unit impulse and a constant
               (all their energy is state carried across chunks); the "gated" signal (both gates drop blocks); a 30 s clip (the
               scan with several chunks per thread); 96 005 samples at 48 kHz (another step length, still whole chunks: 75 C);
               56 445 samples at 44.1 kHz and 30 011 at 24 kHz (steps of 4410 and 2400 samples are no multiple of C: chunks
               straddle step boundaries and their energy is split between two steps); counts = NULL;
               a waveform 4 bytes off 16-byte alignment; a workspace of exactly the reported size between sentinels.
  determinism  the 30 s clip twice and once on a side stream: equal bits.
  gain         targets -16 and -23, out of place and in place; inputs without a loudness come back bit-identical.
  product      tiny models, pool of 4 x 3 s, six sources: BatchConverter off twice, on (-20) == ops.normalize_loudness of the off
               run on both match routes, special_match's file on / level None / switch off, bulk_match's files at -16."""
import pytest
import torch

from tests.gpu_child import check, report_fixture

pytestmark = pytest.mark.gpu
CHILD_TIMEOUT_S = 180        # measured: the child takes 3.4 s on a warm machine (1 s of it the oracle on the 30 s clip); the rest is for a cold torch import
report = report_fixture("loudness_child.py", "loudness", CHILD_TIMEOUT_S, stdout_tail=8000)


def test_loudness_equals_the_fp64_oracle(report):
    check(report, "oracle/", 7 + 7 + 4 + 3 + 2 + 2 * 2 + 1)


def test_loudness_is_bit_stable_from_run_to_run_and_across_streams(report):
    check(report, "determinism/", 1 + 1)


def test_gain_reaches_the_target_and_leaves_silence_alone(report):
    check(report, "gain/", 2 * 2 + 2 + 1)


def test_batch_converter_with_loudness_equals_normalising_its_own_output(report):
    check(report, "product/off-twice", 1)
    check(report, "product/on/", 2)


def test_special_match_writes_the_normalised_waveform_only_when_asked(report):
    check(report, "product/special_match/", 4)


def test_bulk_match_writes_every_file_at_the_target_level(report):
    check(report, "product/bulk_match/", 3)
    check(report, "product/ran", 1)


def test_parent_process_left_the_gpu_alone(report):
    assert not torch.cuda.is_initialized()
