"""GPU: the pool-silence trimmer (knnsvc_vad_trim_seg, ops.vad_trim, the vad_trigger_level / use_vad switches of
get_complete_spk_pool, special_match and serving.TargetVoice) against the fp64 oracle in tests/vad_oracle.py.  Tolerances and
their reasons are in tests/vad_child.py.

The oracle restates the sox `vad` effect with torchaudio's default parameters (include/knnsvc_hip.h) and is the specification;
torchaudio and sox are not available to these tests: parity with torchaudio's own code is not pinned.

All GPU work runs in ONE fresh child interpreter (tests/vad_child.py) that writes a report; the tests only read it.  This module
sorts in front of test_gpu_dist2, which must find the interpreter without an initialised GPU, so nothing here may touch the GPU in
the pytest process.

Cases (tests/vad_cases.py; tests/test_vad_cpu.py shows on the oracle alone that none of their decisions stands closer than 1e-6
to flipping, so measures that agree within 1e-6 must give the oracle's cut points EXACTLY):
  n1599 .. n2400     0, 1, 1 and 2 measurements: the boundaries of the measurement count; all dropped (the boot phase never ends)
  tone2s/3,7,12      0.6 s of noise, a 220 Hz tone with harmonics, noise: 39 measurements, the steady state triggers; three levels,
                     the highest never reached
  early-burst        speech from 0.2 s on: the walk-back ends in the boot's zero measures
  two-bursts/gap3,8  a short burst 3 and 8 quiet measurements ahead of the speech: within and beyond gap_len
  short-voiced       0.3 s of speech: the front cut shortens what the reversed scan may use
  golden-tgt         tests/golden/sample_content/tgt.wav
  tone-8k            the 2 s case at 8 kHz: the constants that follow the rate
  stacked            five recordings of different lengths in ONE call == each alone, bit for bit
  product            seeded small models, a target with a second of near-silence at both ends: fewer pool frames at level 7 than
                     at level 0 (fails without the feature), features / spectrum / harmonics of the hand-trimmed waveform, f0 = the
                     untrimmed file's track sliced, special_match(use_vad=True) keeps the source's length, the level is ignored
                     without the switch, serving.TargetVoice takes the level, a pool without speech is refused"""
import pytest
import torch

from tests.gpu_child import check, report_fixture

pytestmark = pytest.mark.gpu
CHILD_TIMEOUT_S = 180        # measured: the GPU work takes under 3 s; the rest is for a cold torch import
report = report_fixture("vad_child.py", "vad", CHILD_TIMEOUT_S, stdout_tail=8000)


def test_cut_points_equal_the_oracle_exactly(report):
    check(report, "cut/", 4 + 3 + 1 + 2 + 1 + 1 + 1 + 1)          # the twelve 16 kHz cases, the 8 kHz case, the plain call


def test_measures_equal_the_oracle_within_the_margin(report):
    check(report, "measures/", 12 + 1 + 1)
    print("largest |measure - oracle| over all cases:", report["measures/largest-error"]["detail"])


def test_five_recordings_in_one_call_equal_each_alone_bit_for_bit(report):
    check(report, "stacked/", 5)


def test_ops_refuses_bad_levels_shapes_and_rates(report):
    check(report, "refuse/", 3)
    check(report, "oracle/ran", 1)


def test_pool_of_a_trimmed_target_has_fewer_frames(report):
    check(report, "product/pool/fewer-frames", 1)


def test_trimmed_pool_is_the_pool_of_the_hand_trimmed_waveform(report):
    check(report, "product/pool/precondition", 1)
    check(report, "product/pool/features-of-the-hand-trimmed-waveform", 1)
    check(report, "product/pool/f0-is-the-sliced-track", 1)


def test_a_pool_without_speech_is_refused(report):
    check(report, "product/pool/empty-pool-refused", 1)


def test_special_match_keeps_the_source_length_and_ignores_the_level_without_the_switch(report):
    check(report, "product/special_match/", 2)


def test_target_voice_takes_the_level(report):
    check(report, "product/target-voice", 1)
    check(report, "product/ran", 1)


def test_parent_process_left_the_gpu_alone(report):
    assert not torch.cuda.is_initialized()
