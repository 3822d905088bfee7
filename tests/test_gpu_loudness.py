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
import json
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD_TIMEOUT_S = 180        # measured: the child takes 3.4 s on a warm machine (1 s of it the oracle on the 30 s clip); the rest is for a cold torch import


@pytest.fixture(scope="module")
def report(tmp_path_factory):
    if torch.cuda.is_initialized():
        pytest.skip("ranks are spawned from a process that has not initialised the GPU: run this module first / on its own")
    out = str(tmp_path_factory.mktemp("loudness") / "report.json")
    try:
        r = subprocess.run([sys.executable, "tests/loudness_child.py", out], timeout=CHILD_TIMEOUT_S, cwd=ROOT,
                           capture_output=True, text=True)
    except subprocess.TimeoutExpired as e:
        return {"__failed__": f"child timed out after {CHILD_TIMEOUT_S} s\n" + str(e.stderr or "")[-3000:]}
    print(r.stdout[-8000:])
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


def test_loudness_equals_the_fp64_oracle(report):
    _check(report, "oracle/", 7 + 7 + 4 + 3 + 2 + 2 * 2 + 1)


def test_loudness_is_bit_stable_from_run_to_run_and_across_streams(report):
    _check(report, "determinism/", 1 + 1)


def test_gain_reaches_the_target_and_leaves_silence_alone(report):
    _check(report, "gain/", 2 * 2 + 2 + 1)


def test_batch_converter_with_loudness_equals_normalising_its_own_output(report):
    _check(report, "product/off-twice", 1)
    _check(report, "product/on/", 2)


def test_special_match_writes_the_normalised_waveform_only_when_asked(report):
    _check(report, "product/special_match/", 4)


def test_bulk_match_writes_every_file_at_the_target_level(report):
    _check(report, "product/bulk_match/", 3)
    _check(report, "product/ran", 1)


def test_parent_process_left_the_gpu_alone(report):
    assert not torch.cuda.is_initialized()
