"""fp64 numpy restatement of the two output-dynamics definitions of include/knnsvc_hip.h ("Output dynamics"): the envelope mix
and the peak ceiling.  Written from the definitions, not from csrc/dynamics.hip: whole-array numpy, no tiles, no halo, no
doubling.  Also the seeded test signals both test modules share."""
import math

import numpy as np

FLOOR, CAP = 1e-3, 4.0


# ------------------------------------------------------------------ envelope mix
def block_energies(v, T, hop):
    """sum of v[n]^2 over [j hop, (j + 1) hop), j = 0 .. T - 1, v zero-extended or cut to T hop samples."""
    w = np.zeros(T * hop, np.float64)
    m = min(len(v), T * hop)
    w[:m] = np.asarray(v[:m], np.float64)
    return (w * w).reshape(T, hop).sum(axis=1)


def frame_rms(b, hop):
    p = np.concatenate([[0.0], b, [0.0]])
    return np.sqrt((p[:-2] + p[1:-1] + p[2:]) / (3.0 * hop))


def relative_envelope(v, T, hop):
    """max(r[t] / R, 1e-3) of a signal, or None when its global RMS is zero or not finite."""
    b = block_energies(v, T, hop)
    R = math.sqrt(b.sum() / (T * hop)) if np.isfinite(b.sum()) else float("nan")
    if not (R > 0.0 and math.isfinite(R)):
        return None
    return np.maximum(frame_rms(b, hop) / R, FLOOR)


def envelope_gains(y, x, a, hop=320):
    """G [T] fp64, or None when the definition leaves y unchanged (a silent or non-finite signal)."""
    N = len(y)
    assert N % hop == 0 and N > 0
    T = N // hop
    px, py = relative_envelope(x, T, hop), relative_envelope(y, T, hop)
    if px is None or py is None:
        return None
    return np.minimum((px / py) ** a, CAP)


def sample_gains(G, hop):
    T = len(G)
    n = np.arange(T * hop, dtype=np.float64)
    p = (n - hop / 2) / hop
    t0 = np.clip(np.floor(p), 0, T - 1).astype(np.int64)
    t1 = np.minimum(t0 + 1, T - 1)
    f = np.clip(p - t0, 0.0, 1.0)
    return G[t0] + f * (G[t1] - G[t0])


def envelope_mix(y, x, a, hop=320):
    """-> (out fp32, G fp64 [T]); G is all ones where the definition leaves y unchanged."""
    y = np.asarray(y, np.float32)
    G = envelope_gains(y, x, a, hop)
    if G is None:
        return y.copy(), np.ones(len(y) // hop)
    return (y.astype(np.float64) * sample_gains(G, hop)).astype(np.float32), G


# ------------------------------------------------------------------ peak ceiling
def lookahead(sample_rate):
    return int(math.floor(0.005 * sample_rate + 0.5))


def hann(L):
    k = np.arange(-L, L + 1, dtype=np.float64)
    w = 1.0 + np.cos(np.pi * k / (L + 1))
    return w / w.sum()


def limiter_gain(y, peak_db, sample_rate=16000):
    """s [N] fp64 of the definition (k ascending in the smoothing sum)."""
    y = np.asarray(y, np.float32).astype(np.float64)
    N, L = len(y), lookahead(sample_rate)
    c = 10.0 ** (peak_db / 20.0)
    r = np.ones(N + 4 * L)                       # r over [-2L, N + 2L)
    a = np.abs(y)
    over = a > c
    r[2 * L:2 * L + N][over] = c / a[over]
    m = r[:N + 2 * L].copy()                     # m over [-L, N + L): index j + L  <-  min r[j - L .. j + L] = r index j + L .. j + 3L
    for d in range(1, 2 * L + 1):
        np.minimum(m, r[d:d + N + 2 * L], out=m)
    q = 1.0 - m
    h = hann(L)
    acc = np.zeros(N)
    for i in range(2 * L + 1):                   # k = i - L ascending; m[n + k] sits at index n + i
        acc += h[i] * q[i:i + N]
    return 1.0 - acc


def limit_peak(y, peak_db, sample_rate=16000):
    """-> (out fp32, count of samples with s < 1, smallest s (1.0 when none))."""
    y = np.asarray(y, np.float32)
    s = limiter_gain(y, peak_db, sample_rate)
    out = (y.astype(np.float64) * s).astype(np.float32)
    return out, int((s < 1.0).sum()), float(s.min()) if len(s) else 1.0


# ------------------------------------------------------------------ shared signals
def noise(n, seed, amp=0.2):
    return (amp * np.random.default_rng(seed).standard_normal(n)).astype(np.float32)


def sines(n, seed, amp=0.3):
    rng = np.random.default_rng(seed)
    t = np.arange(n) / 16000.0
    v = sum(rng.uniform(0.2, 1.0) * np.sin(2 * np.pi * rng.uniform(80, 3000) * t + rng.uniform(0, 6.28)) for _ in range(5))
    return (amp * v / 3.0).astype(np.float32)


def phrased(T, seed, hop=320, return_bursts=False):
    """Bursts of noisy sines of different amplitudes (0.02 .. 0.6, each with a slow swell) with digital silence between them,
    T hop samples; every burst and every rest is a whole number of blocks, 4 .. 12 blocks long.
    return_bursts: (signal, [(first block, one past the last block) of every burst])."""
    rng = np.random.default_rng(seed)
    v = np.zeros(T * hop, np.float64)
    bursts = []
    j, on = int(rng.integers(0, 3)), True
    while j < T:
        ln = int(rng.integers(4, 13))
        e = min(T, j + ln)
        if on:
            n = (e - j) * hop
            t = np.arange(n) / 16000.0
            amp = rng.uniform(0.02, 0.6)
            swell = 1.0 + 0.5 * np.sin(np.pi * np.arange(n) / n)
            v[j * hop:e * hop] = amp * swell * (np.sin(2 * np.pi * rng.uniform(100, 900) * t) + 0.3 * rng.standard_normal(n))
            bursts.append((j, e))
        j, on = e, not on
    v = v.astype(np.float32)
    return (v, bursts) if return_bursts else v
