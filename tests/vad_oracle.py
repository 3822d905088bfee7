"""fp64 oracle of the pool-silence trimmer (a helper: no test in here).  Pure numpy.

The sox `vad` effect with torchaudio's default parameters, as restated in include/knnsvc_hip.h, applied to both ends of a mono
recording the way ddsp_matcher.py:459-491 applies it (front, then the flipped remainder, every cut a whole number of 320-sample
hops).  That restatement is the specification the device code is held to; torchaudio and sox are not available to these tests, so
parity with torchaudio's own implementation is NOT pinned.

Two formulations of the same definition:
  measures / scan / trim     every measurement of a direction at once (batched FFTs), then a scan for the trigger;
  streaming_start / streaming_trim
                             literal: samples enter a ring buffer of 20 periods + measure_len one by one, a measurement is taken
                             every period from the newest measure_len samples, processing stops at the trigger and the output
                             starts (20 - j*) periods into the buffer."""
import math

import numpy as np

HOP = 320
MEASURES_LEN, GAP_LEN, BOOT_COUNT_MAX, NOISE_REDUCTION = 20, 5, 6, 1.35


def constants(sr):
    """Every constant from the sample rate.  16 kHz: measure_len 1600, dft_len 2048, period 800, s0 6, s1 768, c0 4, c1 53."""
    measure_len = int(sr * 0.1 + .5)
    dft_len = 16
    while dft_len < measure_len:
        dft_len *= 2
    s0 = max(1, int(50.0 / sr * dft_len + .5))
    s1 = min(int(6000.0 / sr * dft_len + .5), dft_len // 2)
    i, j = np.arange(measure_len), np.arange(s1 - s0)
    return dict(measure_len=measure_len, dft_len=dft_len, period=int(sr / 20.0 + .5), s0=s0, s1=s1,
                c0=int(math.ceil(sr * .5 / 2000.0)), c1=min(int(math.floor(sr * .5 / 150.0)), dft_len // 4),
                smooth=math.exp(-1.0 / 8.0), up=math.exp(-1.0 / 2.0), down=math.exp(-5.0), trig=math.exp(-1.0 / 5.0),
                win=2.0 / math.sqrt(measure_len) * (0.5 - 0.5 * np.cos(2.0 * np.pi * i / measure_len)),
                cwin=2.0 / math.sqrt(s1 - s0) * (0.5 - 0.5 * np.cos(2.0 * np.pi * j / (s1 - s0))))


def n_measurements(length, k):
    return (length - k["measure_len"]) // k["period"] + 1 if length >= k["measure_len"] else 0


def _track(a, m, S, N, k):
    """One step of the spectrum / noise-floor recurrences on the bins' magnitudes a -> (S, N, e)."""
    if m < BOOT_COUNT_MAX:
        b = float(m + 1)
        S = (b / (1.0 + b)) * S + (1.0 / (1.0 + b)) * a
        d = S * S
        N = d
    else:
        S = k["smooth"] * S + (1.0 - k["smooth"]) * a
        d = S * S
        mu = np.where(d > N, k["up"], k["down"])
        N = mu * N + (1.0 - mu) * d
    return S, N, np.sqrt(np.maximum(0.0, d - NOISE_REDUCTION * N))


def _measure_of(e, k):
    """e [.., bins] -> measure [..]."""
    c = np.zeros(e.shape[:-1] + (k["dft_len"] // 2,))
    c[..., k["s0"]:k["s1"]] = e * k["cwin"]
    r = (np.abs(np.fft.rfft(c, axis=-1)[..., k["c0"]:k["c1"]]) ** 2).sum(-1)
    with np.errstate(divide="ignore"):
        return np.where(r > 0, np.maximum(0.0, 21.0 + np.log(r / (k["c1"] - k["c0"]))), 0.0)


def measures(x, sr=16000, reverse=False):
    """All M measures of one direction, fp64 [M]."""
    k = constants(sr)
    x = np.asarray(x, np.float64)
    x = x[::-1] if reverse else x
    M = n_measurements(x.size, k)
    if M == 0:
        return np.zeros(0)
    frames = x[np.arange(M)[:, None] * k["period"] + np.arange(k["measure_len"])[None, :]]
    a = np.abs(np.fft.rfft(frames * k["win"], n=k["dft_len"], axis=1)[:, k["s0"]:k["s1"]])
    S = N = np.zeros(k["s1"] - k["s0"])
    e = np.empty_like(a)
    for m in range(M):
        S, N, e[m] = _track(a[m], m, S, N, k)
    return _measure_of(e, k)


def _walk_back(window, level):
    """window[j] = the measure j measurements before the trigger (0 before the recording) -> j*"""
    jt = jz = MEASURES_LEN
    for j in range(MEASURES_LEN):
        v = window[j]
        if v >= level and j <= jt + GAP_LEN:
            jz = jt = j
        elif v == 0 and jt >= jz:
            jz = j
    return min(MEASURES_LEN, jz)


def scan(meas, level, period, details=False):
    """First sample to keep, -1 when nothing fires.  details: (start, dict(m, means up to the trigger, walked-back window))."""
    trig = math.exp(-1.0 / 5.0)
    mean, means = 0.0, []
    for m in range(len(meas)):
        mean = trig * mean + (1.0 - trig) * meas[m]
        means.append(mean)
        if mean >= level:
            window = [meas[m - j] if m - j >= 0 else 0.0 for j in range(MEASURES_LEN)]
            start = max(0, m - _walk_back(window, level)) * period
            return (start, dict(m=m, means=means, window=window)) if details else start
    return (-1, dict(m=None, means=means, window=[])) if details else -1


def _round_up(v):
    return (v + HOP - 1) // HOP * HOP


def trim(x, level, sr=16000, details=False):
    """(lstrip, rstrip), (-1, -1) for a dropped recording.  details: also dict(fwd, rev: all measures of the direction,
    m_rev: measurements the reversed scan may use, margin: the smallest distance of any decision from flipping, see margin())."""
    k = constants(sr)
    L = len(x)
    fwd, rev = measures(x, sr), measures(x, sr, reverse=True)
    start, df = scan(fwd, level, k["period"], details=True)
    info = dict(fwd=fwd, rev=rev, m_rev=0, margin=_margin(df, level))
    res = (-1, -1)
    if start >= 0:
        l = _round_up(start)
        info["m_rev"] = n_measurements(L - l, k)
        rstart, dr = scan(rev[:info["m_rev"]], level, k["period"], details=True)
        info["margin"] = min(info["margin"], _margin(dr, level))
        if rstart >= 0 and L - l - _round_up(rstart) >= k["measure_len"]:
            res = (l, _round_up(rstart))
    return (res, info) if details else res


def _margin(d, level):
    """How far the scan's decisions are from flipping: the smallest of |mean - level| at every step up to the trigger,
    |meas - level| of every walked-back entry, and every walked-back entry that is not exactly 0 (the `== 0` test); inf when
    there is nothing to decide.  Measures that agree within less than this give the same cut points."""
    vals = [abs(v - level) for v in d["means"]] + [abs(v - level) for v in d["window"]]
    vals += [v for v in d["window"] if v != 0.0]
    return min(vals) if vals else math.inf


# ------------------------------------------------------------------ the literal streaming formulation
def streaming_start(x, level, sr=16000):
    """First sample to keep (-1: never triggered), one sample at a time."""
    k = constants(sr)
    ml, period = k["measure_len"], k["period"]
    x = np.asarray(x, np.float64)
    n_buf = MEASURES_LEN * period + ml
    buf, at = np.zeros(n_buf), 0
    ring, ri = np.zeros(MEASURES_LEN), 0
    timer, count, mean, trig = ml, 0, 0.0, k["trig"]
    S = N = np.zeros(k["s1"] - k["s0"])
    newest = np.arange(ml)
    for pos in range(x.size):
        buf[at] = x[pos]
        at = (at + 1) % n_buf
        timer -= 1
        if timer:
            continue
        timer = period
        frame = buf[(at - ml + newest) % n_buf]
        a = np.abs(np.fft.rfft(frame * k["win"], n=k["dft_len"])[k["s0"]:k["s1"]])
        S, N, e = _track(a, count, S, N, k)
        count += 1
        ring[ri] = float(_measure_of(e, k))
        mean = trig * mean + (1.0 - trig) * ring[ri]
        if mean >= level:
            jstar = _walk_back([ring[(ri - j) % MEASURES_LEN] for j in range(MEASURES_LEN)], level)
            flushed = (MEASURES_LEN - jstar) * period                # dropped from the front of the buffer
            return max(0, pos + 1 - n_buf + flushed)
        ri = (ri + 1) % MEASURES_LEN
    return -1


def streaming_trim(x, level, sr=16000):
    k = constants(sr)
    x = np.asarray(x, np.float64)
    start = streaming_start(x, level, sr)
    if start < 0:
        return (-1, -1)
    l = _round_up(start)
    rstart = streaming_start(x[l:][::-1], level, sr)
    if rstart < 0 or x.size - l - _round_up(rstart) < k["measure_len"]:
        return (-1, -1)
    return (l, _round_up(rstart))
