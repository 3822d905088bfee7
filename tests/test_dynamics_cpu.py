"""CPU: output dynamics.  (1) The properties the definitions of include/knnsvc_hip.h promise, on their fp64 numpy restatement
tests/dynamics_oracle.py (the yardstick of tests/test_gpu_dynamics.py); (2) the host logic: matching.resolve_dynamics and its
call at the top of every entry point, before a file is touched."""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dynamics_oracle as O  # noqa: E402

L = 80                      # look-ahead at 16 kHz
HOP = 320


# ------------------------------------------------------------------ peak ceiling
def test_lookahead_is_5_ms_rounded():
    assert [O.lookahead(sr) for sr in (8000, 16000, 22050, 24000, 44100, 48000)] == [40, 80, 110, 120, 221, 240]
    assert all(O.lookahead(sr) == (sr + 100) // 200 for sr in range(8000, 48001))      # the library's integer form
    h = O.hann(L)
    assert len(h) == 2 * L + 1 and h.min() > 0 and abs(h.sum() - 1) < 1e-15
    assert abs((1 + np.cos(np.pi * np.arange(-L, L + 1) / (L + 1))).sum() - (2 * L + 2)) < 1e-10      # the closed-form divisor


@pytest.mark.parametrize("n", [1, 2, L, L + 1, 2 * L, 2 * L + 1, 4 * L + 1, 1000, 5000])
@pytest.mark.parametrize("p", [0.0, -1.0, -6.0])
def test_ceiling_holds_after_the_one_rounding(n, p):
    c = 10.0 ** (p / 20.0)
    y = O.noise(n, 7 + n, amp=0.8)
    assert np.abs(y).max() > c or n < 3
    out, count, smin = O.limit_peak(y, p)
    assert np.abs(out.astype(np.float64)).max() <= c * (1 + 2.0 ** -23)
    assert 0 < smin <= 1 and 0 <= count <= n


@pytest.mark.parametrize("n", [1, L, 2 * L + 1, 5000])
def test_a_signal_under_the_ceiling_comes_back_bit_identical(n):
    y = np.clip(O.noise(n, 11 + n), -0.49, 0.49)
    out, count, smin = O.limit_peak(y, 20 * math.log10(0.5))
    assert np.array_equal(out.view(np.int32), y.view(np.int32)) and count == 0 and smin == 1.0


@pytest.mark.parametrize("at", [0, 1, 2 * L - 1, 2 * L, 1700, 4999 - 2 * L, 4999])
def test_a_single_peak_touches_4L_plus_1_samples_and_the_minimum_gain_is_c_over_peak(at):
    n, c, peak = 5000, 0.5, 0.9
    y = np.clip(O.noise(n, 3), -0.4, 0.4)
    y[at] = -peak if at % 2 else peak
    s = O.limiter_gain(y, 20 * math.log10(c))
    touched = np.nonzero(s < 1.0)[0]
    lo, hi = max(0, at - 2 * L), min(n - 1, at + 2 * L)
    assert touched[0] == lo and touched[-1] == hi and len(touched) == hi - lo + 1
    if 2 * L <= at <= n - 1 - 2 * L:
        assert len(touched) == 4 * L + 1
    cq = 10.0 ** (20 * math.log10(c) / 20.0)
    assert abs(s.min() / (cq / np.float64(np.float32(peak))) - 1) < 1e-15 and s.argmin() == at
    out, _, _ = O.limit_peak(y, 20 * math.log10(c))
    untouched = np.ones(n, bool)
    untouched[lo:hi + 1] = False
    assert np.array_equal(out[untouched].view(np.int32), y[untouched].view(np.int32))


def test_a_plateau_and_a_signal_entirely_over_the_ceiling_get_c_over_level():
    c = 0.5
    p = 20 * math.log10(c)
    y = np.zeros(3000, np.float32)
    y[1000:2000] = 0.9
    s = O.limiter_gain(y, p)
    want = 10.0 ** (p / 20.0) / np.float64(np.float32(0.9))
    assert np.allclose(s[1000 + L:2000 - L], want, rtol=1e-14, atol=0)
    s = O.limiter_gain(np.full(3000, 0.9, np.float32), p)
    assert np.allclose(s[2 * L:-2 * L], want, rtol=1e-14, atol=0) and s.max() < 1


# ------------------------------------------------------------------ envelope mix
def test_mix_zero_gives_unit_gains_and_silence_leaves_y_alone():
    y, x = O.sines(20 * HOP, 1), O.phrased(20, 2)
    out, G = O.envelope_mix(y, x, 0.0)
    assert np.all(G == 1.0) and np.array_equal(out.view(np.int32), y.view(np.int32))
    for yy, xx in ((y, np.zeros_like(x)), (np.zeros_like(y), x), (y, np.zeros(0, np.float32))):
        out, G = O.envelope_mix(yy, xx, 0.7)
        assert np.all(G == 1.0) and np.array_equal(out.view(np.int32), yy.view(np.int32))


def test_full_mix_transfers_the_shape_of_the_source_envelope():
    """a = 1: the output's relative envelope, re-measured, is the source's up to one constant — on the interior frames of every
    burst of the phrased source (the three blocks of the frame inside one burst; at the edges of a burst the linear
    interpolation between a burst frame and a rest frame is what the definition asks for, not the source's envelope).
    Measured with this seed: spread max |ratio / median - 1| = 0.0782 (the output's blocks carry y's own fluctuation and
    the gain is a line between frame centres, not a step); the bound is that rounded up to one digit."""
    T = 200
    x, bursts = O.phrased(T, 5, return_bursts=True)
    y = O.sines(T * HOP, 6)
    out, G = O.envelope_mix(y, x, 1.0)
    assert G.max() <= O.CAP
    p_out, p_x = O.relative_envelope(out, T, HOP), O.relative_envelope(x, T, HOP)
    inner = np.array([t for a, b in bursts for t in range(a + 1, b - 1)])
    assert len(inner) > 40
    ratio = p_out[inner] / p_x[inner]
    spread = float(np.abs(ratio / np.median(ratio) - 1).max())
    print("spread", spread)
    assert spread <= 0.08
    # and the rests became rests: a frame whose samples are all scaled by floor gains (the source's envelope on the floor two
    # frames to either side) ends about 60 dB under the average
    rest = np.array([t for t in range(2, T - 2) if np.all(p_x[t - 2:t + 3] == O.FLOOR)])
    rest_ratio = p_out[rest] / p_x[rest] / np.median(ratio)
    print("rests", len(rest), float(np.abs(rest_ratio - 1).max()))
    assert len(rest) > 10 and np.abs(rest_ratio - 1).max() <= 0.08          # the same constant, within the same spread


def test_level_invariance_is_exact_when_the_scaling_is():
    T = 30
    y = O.sines(T * HOP, 8)
    m = np.round(O.phrased(T, 9).astype(np.float64) * 0.1 * 2 ** 20)          # |m| < 2^17: m / 2^20 and 100 m / 2^20 are both fp32
    lo, hi = (m / 2 ** 20).astype(np.float32), (100 * m / 2 ** 20).astype(np.float32)
    assert np.array_equal(hi.astype(np.float64), 100 * lo.astype(np.float64))
    g_lo, g_hi = O.envelope_gains(y, lo, 0.5), O.envelope_gains(y, hi, 0.5)
    assert np.allclose(g_lo, g_hi, rtol=1e-14, atol=0)


def test_cap_and_floor_are_reached():
    T = 40
    rng = np.random.default_rng(4)
    x = (0.2 * rng.standard_normal(T * HOP)).astype(np.float32)
    y = (0.2 * rng.standard_normal(T * HOP)).astype(np.float32)
    y[10 * HOP:16 * HOP] *= 1e-2                # the generator left these frames 40 dB low: the gain would be 100, capped at 4
    G = O.envelope_gains(y, x, 1.0)
    assert np.all(G[11:15] == O.CAP) and G.max() == O.CAP
    x[25 * HOP:31 * HOP] = 0.0                  # a rest in the source: its relative envelope sits on the floor
    px, py = O.relative_envelope(x, T, HOP), O.relative_envelope(y, T, HOP)
    assert np.all(px[26:30] == O.FLOOR)
    G = O.envelope_gains(y, x, 1.0)
    assert np.allclose(G[26:30], O.FLOOR / py[26:30], rtol=1e-14) and np.all(G[26:30] < 2e-3)


def test_gain_is_linear_between_frame_centres_and_constant_outside():
    G = np.array([1.0, 3.0, 2.0])
    g = O.sample_gains(G, 64)
    assert np.all(g[:33] == 1.0) and g[32 + 64] == 3.0 and g[32 + 32] == 2.0 and np.all(g[32 + 128:] == 2.0) and len(g) == 192


# ------------------------------------------------------------------ host logic
def test_resolve_dynamics():
    from knn_svc_amd.matching import resolve_dynamics
    assert resolve_dynamics(None, None) == (0.0, None) and resolve_dynamics(0, 0) == (0.0, 0.0)
    assert resolve_dynamics(np.float32(0.5), -3) == (0.5, -3.0) and resolve_dynamics(1, np.float64(-0.1)) == (1.0, -0.1)
    for bad in (-0.01, 1.01, float("nan"), float("inf"), "0.5", True, [0.5]):
        with pytest.raises(ValueError, match="envelope_mix"):
            resolve_dynamics(bad, None)
    for bad in (0.1, float("nan"), float("inf"), float("-inf"), "-1", False, (-1,)):
        with pytest.raises(ValueError, match="peak_db"):
            resolve_dynamics(0.0, bad)


def _bare_vc():
    from knn_svc_amd.matcher import KNeighborsVC
    return KNeighborsVC.__new__(KNeighborsVC)          # no models, no device: the checks under test come before either is used


@pytest.mark.parametrize("kw", [dict(envelope_mix=1.5), dict(peak_db=3.0), dict(envelope_mix=float("nan")), dict(peak_db="x")])
def test_every_entry_point_refuses_a_bad_value_before_it_touches_a_file(kw, tmp_path):
    from knn_svc_amd import serving
    from knn_svc_amd.inference import main
    vc, gone = _bare_vc(), str(tmp_path / "no" / "such.wav")
    with pytest.raises(ValueError, match="envelope_mix|peak_db"):
        vc.special_match(gone, gone, **kw)
    with pytest.raises(ValueError, match="envelope_mix|peak_db"):
        vc.bulk_match(gone, gone, gone, **kw)
    with pytest.raises(ValueError, match="envelope_mix|peak_db"):
        vc.many_to_one([gone], gone, **kw)
    with pytest.raises(ValueError, match="envelope_mix|peak_db"):
        serving.BatchConverter(vc, None, **kw)
    if not isinstance(next(iter(kw.values())), str):
        with pytest.raises(SystemExit) as e:           # argparse's error exit, before the models are loaded
            main([gone, gone] + [f"--{k}={v}" for k, v in kw.items()])
        assert e.value.code == 2
    assert not (tmp_path / "no").exists()


def test_vocode_refuses_an_envelope_mix_without_the_source():
    import torch
    with pytest.raises(ValueError, match="src_wav"):
        _bare_vc().vocode(torch.zeros(1, 2, 4), torch.zeros(1, 2, 1), envelope_mix=0.5)


def test_cli_defaults_are_off():
    from knn_svc_amd.inference import build_parser
    a = build_parser().parse_args(["s", "t"])
    assert a.envelope_mix == 0.0 and a.peak_db is None
    a = build_parser().parse_args(["s", "t", "--envelope_mix", "0.7", "--peak_db", "-1"])
    assert a.envelope_mix == 0.7 and a.peak_db == -1.0


def test_a_three_argument_vocode_fn_is_told_apart_from_a_four_argument_one():
    """The tail asks for the source (``needs_source``) exactly when the envelope mix is on; a plain three-argument callable has
    no such attribute and is called with the three arguments (matching.vocoding_tail)."""
    from knn_svc_amd.matcher import Tail
    from knn_svc_amd.matching import vocoding_tail
    from knn_svc_amd.options import Extensions
    vc = _bare_vc()
    tail = lambda f0only, loudness_db=None, envelope_mix=0.0, peak_db=None: Tail(vc, f0only, Extensions.from_serving(
        loudness_db=loudness_db, envelope_mix=envelope_mix, peak_db=peak_db))
    assert not tail(False).needs_source and not tail(True, -16.0, 0.0, -1.0).needs_source
    assert tail(False, None, 0.5).needs_source and tail(True, None, 0.5, -1.0).needs_source
    loaded = []
    plain = vocoding_tail(lambda c, f0, h: (c, f0, h), ["a"], loaded.append)
    assert plain("a", (1, 2, 3)) == (1, 3, 2) and loaded == []

    def wants(c, f0, h, src_wav=None):
        return c, f0, h, src_wav
    wants.needs_source = True
    sourced = vocoding_tail(wants, ["a", "b"], lambda it: (loaded.append(it), it.upper())[1])
    assert loaded == ["a", "b"] and sourced("b", (1, 2, 3)) == (1, 3, 2, "B")
