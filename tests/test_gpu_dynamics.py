"""GPU: output dynamics (knnsvc_envelope_mix / knnsvc_peak_limit, ops.envelope_mix / ops.limit_peak, the envelope_mix / peak_db
switches of special_match, bulk_match, many_to_one's serving.BatchConverter and a RequestQueue in front of it) against the fp64
oracle in tests/dynamics_oracle.py.  Tolerances and their reasons are in tests/dynamics_child.py.

All GPU work runs in ONE fresh child interpreter (tests/dynamics_child.py) that writes a report; the tests only read it.  This
module sorts in front of test_gpu_dist2, which must find the interpreter without an initialised GPU, so nothing here may touch
the GPU in the pytest process.

Cases (the smallest sizes that reach every path and boundary; tile = samples per workgroup and L = 80, the look-ahead at 16 kHz,
read from the library: ops.peak_limit_layout):
  envelope     T = 1, 2, 3, 64 at hop 320 and T = 5 at hop 64; a source one sample, one block and half the length short, and a
               longer one; the phrased source at a = 0.25, 0.5, 1; a silent source, a silent output, an empty source (y bit for
               bit); a source 40 dB lower (an exact scaling) against the same at equal level; in place; gains = NULL; pointers
               4 bytes off 16-byte alignment; a workspace of exactly the reported size between sentinels, one byte less refused;
               n no multiple of hop and hop = 100 are error codes and launch nothing.
  ceiling      lengths 0, 1, L, L+1, 2L, 2L+1, 4L+1, tile-1, tile, tile+1, 3 tile+L+1; single peaks at 0, n-1, tile-1, tile,
               tile-2L, tile+2L (the halo's far ends); two peaks 2L and 2L+1 apart; a negative peak; a plateau across a tile
               boundary; everything over; 44.1 kHz (L = 221); p = 0, -1, -6; identity; in place; misaligned; stats = NULL; bad rate
               and bad level are error codes and launch nothing.
  determinism  a 30 s clip through both twice and once on a side stream: equal bits.
  product      tiny models, pool of 4 x 3 s, six phrased sources: BatchConverter off twice; on (0.7, ceiling at half the off run's
               peak) == the ops by hand on both match routes; with loudness -20 the order mix, loudness, ceiling; a RequestQueue;
               special_match's file on / defaults / normalised past full scale under the ceiling; bulk_match's files."""
import pytest
import torch

from tests.gpu_child import check, report_fixture

pytestmark = pytest.mark.gpu
CHILD_TIMEOUT_S = 240        # the child's own work is a few seconds; the rest is for a cold torch import
report = report_fixture("dynamics_child.py", "dynamics", CHILD_TIMEOUT_S)


def test_envelope_mix_equals_the_fp64_oracle(report):
    check(report, "envelope/T", 5)
    check(report, "envelope/source-", 4)
    check(report, "envelope/phrased-", 3)
    check(report, "envelope/max-error", 1)
    print(report["envelope/max-error"]["detail"])


def test_envelope_mix_leaves_y_alone_when_a_signal_is_silent(report):
    check(report, "envelope/silent-", 4)
    check(report, "envelope/empty-source", 1)


def test_envelope_mix_does_not_depend_on_the_source_level(report):
    check(report, "envelope/level/", 3)


def test_envelope_mix_call_forms_and_refusals(report):
    for name in ("in-place", "gains-null", "pointers-4-bytes-off-alignment", "exact-workspace", "short-workspace-refused",
                 "bad-length-and-bad-hop-are-error-codes"):
        check(report, "envelope/" + name, 1)
    check(report, "envelope/ran", 1)


def test_peak_ceiling_equals_the_fp64_oracle_and_holds_the_ceiling(report):
    check(report, "ceiling/length/", 11)
    check(report, "ceiling/peak-at/", 12)
    check(report, "ceiling/two-peaks/", 2)
    for name in ("negative-peak", "plateau-across-a-tile-boundary", "everything-over", "44100-Hz", "p0", "p-1", "p-6", "several", "max-error"):
        check(report, "ceiling/" + name, 1)
    print(report["ceiling/max-error"]["detail"])


def test_peak_ceiling_returns_a_signal_under_it_bit_identical(report):
    check(report, "ceiling/identity", 1)


def test_peak_ceiling_call_forms_and_refusals(report):
    for name in ("in-place", "pointers-4-bytes-off-alignment", "stats-null", "bad-rate-and-bad-level-are-error-codes", "ran"):
        check(report, "ceiling/" + name, 1)


def test_both_ops_are_bit_stable_from_run_to_run_and_across_streams(report):
    check(report, "determinism/", 1 + 1)


def test_batch_converter_with_dynamics_equals_the_ops_applied_to_its_own_output(report):
    check(report, "product/off-twice", 1)
    check(report, "product/on/", 3)


def test_the_tail_runs_mix_then_loudness_then_ceiling(report):
    check(report, "product/order/", 2)


def test_request_queue_inherits_the_converters_dynamics(report):
    check(report, "product/request-queue", 1)


def test_special_match_writes_the_processed_waveform_only_when_asked(report):
    check(report, "product/special_match/", 4)


def test_bulk_match_writes_every_file_under_the_ceiling(report):
    check(report, "product/bulk_match/", 3)
    check(report, "product/ran", 1)


def test_parent_process_left_the_gpu_alone(report):
    assert not torch.cuda.is_initialized()
