"""numpy fp64 restatement of "Time scale" in include/knnsvc_hip.h (the reference for knnsvc_time_scale_seg) and of
matching.duration_plan.  The source index is one fused multiply-add (evaluated exactly and rounded once); every other step is an
fp64 operation rounded on its own (numpy never contracts); the features are rounded to fp32 once at the end, as the kernel does,
so the comparison with the device is bit for bit.

    taps(T, T_out, c)          -> i0, i1 (int64), l0, l1 (fp64) per output row
    features(x, T_out, c)      -> fp64 [T_out, dim] (before the final rounding); features32: rounded to fp32
    f0(f, T_out, c)            -> fp32 [T_out]
    time_scale_seg(x, f, seg, out_frames, inv_scales) -> the stacked call, segment by segment
    duration_plan(T, seconds)  -> (T_out, inv_scale), upstream's arithmetic
"""
import math
from fractions import Fraction

import numpy as np

SCALE_MIN, SCALE_MAX = 0.25, 4.0


def fma_index(c, T_out):
    """fma(c, j + 0.5, -0.5) for j = 0 .. T_out - 1, rounded ONCE: the exact rational value, then one conversion to fp64
    (numpy has no fused multiply-add; Fraction -> float is correctly rounded)."""
    c = Fraction(float(c))
    return np.array([float(c * Fraction(2 * j + 1, 2) - Fraction(1, 2)) for j in range(int(T_out))], dtype=np.float64).reshape(-1)


def taps(T, T_out, c):
    r = fma_index(c, T_out)
    r = np.where(r < 0, 0.0, r)
    i0 = r.astype(np.int64)                       # truncation; r >= 0
    i1 = i0 + (i0 < T - 1)
    l1 = r - i0.astype(np.float64)
    over = i0 > T - 1                             # possible only through rounding
    i0 = np.where(over, T - 1, i0); i1 = np.where(over, T - 1, i1); l1 = np.where(over, 0.0, l1)
    return i0, i1, 1.0 - l1, l1


def features(x, T_out, c):
    x = np.asarray(x)
    i0, i1, l0, l1 = taps(x.shape[0], T_out, c)
    a = l0[:, None] * x[i0].astype(np.float64)
    b = l1[:, None] * x[i1].astype(np.float64)
    return a + b


def features32(x, T_out, c):
    return features(x, T_out, c).astype(np.float32)


def f0(f, T_out, c):
    f = np.asarray(f, np.float32)
    i0, i1, l0, l1 = taps(f.shape[0], T_out, c)
    fa, fb = f[i0], f[i1]
    near = np.where(l1 > 0.5, fb, fa)             # a tie goes left
    both = (fa > 0) & (fb > 0)
    with np.errstate(divide="ignore", invalid="ignore"):
        la = l0 * np.log(fa.astype(np.float64))
        lb = l1 * np.log(fb.astype(np.float64))
        glide = np.exp(la + lb).astype(np.float32)
    out = np.where(both, glide, near).astype(np.float32)
    out[near <= 0] = 0.0
    return out


def time_scale_seg(x, f, seg, out_frames, inv_scales):
    xs, fs = [], []
    for s, (n, c) in enumerate(zip(out_frames, inv_scales)):
        a, b = seg[s], seg[s + 1]
        if x is not None:
            xs.append(features32(x[a:b], n, c))
        if f is not None:
            fs.append(f0(f[a:b], n, c))
    return (np.concatenate(xs, 0) if xs else None), (np.concatenate(fs, 0) if fs else None)


def duration_plan(T, target_duration, sr=16000, hop=320):
    target_samples = int(target_duration * sr)
    s = (target_samples / hop) / T
    T_out = int(math.floor(float(T) * s))
    if T_out < 1 or not SCALE_MIN <= s <= SCALE_MAX:
        raise ValueError((T, target_duration, s, T_out))
    return T_out, 1.0 / s


def plan_for_scale(T, s):
    """(T_out, inv_scale) the way F.interpolate derives them from a scale factor: for kernel cases given as a scale."""
    return int(math.floor(float(T) * s)), 1.0 / s


# ---------------------------------------------------------------- inputs of the GPU cases (seeded; tests/test_duration_cpu.py pins them)
def track(n, base_hz, seed, voiced=0.7, run=9):
    """A synthetic f0 track: a slow melody around ``base_hz`` with RESTS — unvoiced runs of about ``run`` frames as exact zeros,
    so that notes have edges on both sides."""
    rng = np.random.default_rng(seed)
    semis = 4.0 * np.sin(np.arange(n) * 0.013 + rng.uniform(0, 6)) + 0.3 * rng.standard_normal(n)
    f = (base_hz * 2.0 ** (semis / 12.0)).astype(np.float32)
    gate = np.repeat(rng.uniform(size=n // run + 1) > voiced, run)[:n]
    f[gate] = 0.0
    return f


def feats(T, dim, seed):
    return np.random.default_rng(seed).standard_normal((T, dim)).astype(np.float32)


def ulp_distance(a, b):
    """Distance in representable fp32 values between two arrays of positive finite floats."""
    return np.abs(np.asarray(a, np.float32).view(np.int32).astype(np.int64) - np.asarray(b, np.float32).view(np.int32).astype(np.int64))
