"""fp64 oracle of the loudness measure (a helper: no test in here).  Pure numpy, the recurrences as plain loops.

Integrated loudness of a mono signal after ITU-R BS.1770-4 with the constants and biquad forms torchaudio.functional.loudness
uses (the definition in include/knnsvc_hip.h, restated): K-weighting = high-shelf (+4 dB, 1500 Hz, Q = 1/sqrt 2) then high-pass
(38 Hz, Q = 0.5), both direct form with zero initial state and NO clamping of the intermediate signals; blocks of G = 0.4 sr
samples every S = G / 4; absolute gate at -70, relative gate 10 below the mean of what the absolute gate kept.

Checked once against scipy.signal.lfilter (filter outputs equal to 2e-13); scipy is not needed to use it."""
import math

import numpy as np


def coefficients(sr):
    """-> ((b, a) shelf, (b, a) high-pass), each divided by a0, fp64."""
    w0 = 2.0 * math.pi * 1500.0 / sr
    A = 10.0 ** (4.0 / 40.0)
    al = math.sin(w0) / (2.0 / math.sqrt(2.0))
    cw = math.cos(w0)
    t = 2.0 * math.sqrt(A) * al
    b = np.array([A * ((A + 1) + (A - 1) * cw + t), -2 * A * ((A - 1) + (A + 1) * cw), A * ((A + 1) + (A - 1) * cw - t)])
    a = np.array([(A + 1) - (A - 1) * cw + t, 2 * ((A - 1) - (A + 1) * cw), (A + 1) - (A - 1) * cw - t])
    shelf = (b / a[0], a / a[0])
    w0 = 2.0 * math.pi * 38.0 / sr
    al = math.sin(w0) / (2.0 * 0.5)
    cw = math.cos(w0)
    b = np.array([(1 + cw) / 2, -(1 + cw), (1 + cw) / 2])
    a = np.array([1 + al, -2 * cw, 1 - al])
    return shelf, (b / a[0], a / a[0])


def biquad(b, a, x):
    """y[i] = b0 x[i] + b1 x[i-1] + b2 x[i-2] - a1 y[i-1] - a2 y[i-2], zero initial state."""
    b0, b1, b2 = (float(v) for v in b)
    a1, a2 = float(a[1]), float(a[2])
    ff = b0 * x
    ff[1:] += b1 * x[:-1]
    ff[2:] += b2 * x[:-2]
    y = ff.tolist()
    y1 = y2 = 0.0
    for i, f in enumerate(y):
        v = f - a1 * y1 - a2 * y2
        y[i] = v
        y2, y1 = y1, v
    return np.asarray(y, np.float64)


def k_weight(x, sr):
    shelf, hp = coefficients(sr)
    return biquad(*hp, biquad(*shelf, np.asarray(x, np.float64)))


def block_levels(x, sr):
    """-> (e [nb] block mean squares, l [nb] block levels)"""
    assert sr % 10 == 0
    G = (4 * sr) // 10
    S = G // 4
    x = np.asarray(x, np.float64).reshape(-1)
    n = x.shape[0]
    nb = (n - G) // S + 1 if n >= G else 0
    if nb == 0:
        return np.zeros(0), np.zeros(0)
    y2 = k_weight(x, sr) ** 2
    e = np.array([y2[j * S:j * S + G].mean() for j in range(nb)])
    with np.errstate(divide="ignore"):
        return e, -0.691 + 10.0 * np.log10(e)


def loudness(x, sr=16000, details=False):
    """-> lkfs (float, -inf when there is no block or a gate leaves nothing); details: (lkfs, (blocks, kept by the absolute
    gate, kept by both), margin) with margin = the least distance in dB of any block level from -70 and from the relative
    threshold (inf where there is none)."""
    e, l = block_levels(x, sr)
    keep1 = l > -70.0
    lk, gamma, n2 = -math.inf, None, 0
    if keep1.any():
        gamma = -0.691 + 10.0 * math.log10(e[keep1].mean()) - 10.0
        keep2 = keep1 & (l > gamma)
        n2 = int(keep2.sum())
        if n2:
            lk = -0.691 + 10.0 * math.log10(e[keep2].mean())
    if not details:
        return lk
    fin = l[np.isfinite(l)]
    margin = math.inf
    if fin.size:
        margin = float(np.abs(fin + 70.0).min())
        if gamma is not None:
            margin = min(margin, float(np.abs(fin - gamma).min()))
    return lk, (int(e.shape[0]), int(keep1.sum()), n2), margin


def gated_signal():
    """The "gated" anchor: 16 kHz, 48013 samples, a silent stretch (absolute gate) and a quiet one (relative gate)."""
    n = 48013
    t = np.arange(n) / 16000.0
    x = 0.3 * np.sin(2 * np.pi * 220 * t) + 0.1 * np.sin(2 * np.pi * 2500 * t + 1) + 0.01 * np.random.default_rng(0).standard_normal(n)
    env = np.ones(n)
    env[12800:24000] = 0.0
    env[32000:41600] = 0.03
    return (x * env).astype(np.float32)
