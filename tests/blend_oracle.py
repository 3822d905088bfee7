"""numpy fp64 restatement of "Voice blend" (points 2 to 4) in include/knnsvc_hip.h: the reference for knnsvc_blend_seg and for the
pool median knnsvc_shift_f0_seg_blend shifts towards.  Every product and every sum is a numpy operation of its own on float64
arrays (numpy never fuses a multiply with an add), the voices go in ascending order, the sum starts with the first product, a
voice whose weight is exactly 0 is not looked at, and a single non-zero weight copies its voice bit for bit.

    normalise(a)                 -> the weights as matching.resolve_blend hands them on: a / math.fsum(a)
    check_row(a)                 -> None, or why the library refuses the row (point 4)
    blend(xs, a)                 -> float32 array: point 2 for one weight row
    blend_seg(xs, seg, rows)     -> the stacked call, segment by segment
    median(pms, a)               -> float32: point 3's pool median
"""
import math

import numpy as np

MAX_VOICES = 4


def normalise(a):
    a = [float(w) + 0.0 for w in a]
    total = math.fsum(a)
    return tuple(w / total for w in a)


def check_row(a):
    a = [float(w) for w in a]
    if not 2 <= len(a) <= MAX_VOICES:
        return "voices"
    if any(not (math.isfinite(w) and w >= 0) for w in a):
        return "entry"
    if not any(w > 0 for w in a):
        return "no positive"
    s = 0.0
    for w in a:
        s += w
    return None if abs(s - 1.0) <= 1e-6 else "sum"


def blend(xs, a):
    """xs: V float32 arrays of one shape; a: V weights.  The arrays of zero-weight voices are not touched."""
    assert len(xs) == len(a) and check_row(a) is None, (len(xs), a)
    live = [v for v in range(len(a)) if float(a[v]) != 0.0]
    if len(live) == 1:
        return np.array(xs[live[0]], dtype=np.float32, copy=True)
    acc = None
    with np.errstate(invalid="ignore", over="ignore"):
        for v in live:
            p = np.float64(a[v]) * np.asarray(xs[v], np.float32).astype(np.float64)      # one multiply
            acc = p if acc is None else acc + p                                          # one add
        return acc.astype(np.float32)                                                    # one rounding


def blend_seg(xs, seg, rows):
    out = np.empty_like(np.asarray(xs[0], np.float32))
    for s in range(len(seg) - 1):
        a, b = seg[s], seg[s + 1]
        out[a:b] = blend([x[a:b] for x in xs], rows[s])
    return out


def median(pms, a):
    """The blended fp32 pool median of a segment from the voices' fp32 medians."""
    return np.float32(blend([np.asarray([m], np.float32) for m in pms], a)[0])


# ---------------------------------------------------------------- test data
def feats(n, dim, seed):
    return np.random.default_rng(seed).standard_normal((n, dim)).astype(np.float32)


def track(n, base_hz, seed, voiced=0.7, run=9):
    """A synthetic f0 track: a slow melody around ``base_hz`` with rests (unvoiced runs of about ``run`` frames as exact zeros)."""
    rng = np.random.default_rng(seed)
    semis = 4.0 * np.sin(np.arange(n) * 0.013 + rng.uniform(0, 6)) + 0.3 * rng.standard_normal(n)
    f = (base_hz * 2.0 ** (semis / 12.0)).astype(np.float32)
    f[np.repeat(rng.uniform(size=n // run + 1) > voiced, run)[:n]] = 0.0
    return f


def table(lens):
    seg = [0]
    for n in lens:
        seg.append(seg[-1] + int(n))
    return seg
