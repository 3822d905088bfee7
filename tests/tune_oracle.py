"""numpy restatement of the section "Pitch correction" of include/knnsvc_hip.h: the reference for knnsvc_tune_f0_seg.  fp64
everywhere, every step rounded on its own (numpy never contracts), the output rounded once to fp32.  The shifted f0 is an INPUT:
the GPU tests feed the device's own, so what is compared is the correction, not the shift.

    tune(f0, seg, tunings) -> (corrected f0 float32, notes int32, smallest decision margin in semitones)

``tunings``: per segment None (off) or anything with ``mask`` / ``strength`` / ``alpha`` / ``log_ref`` (options.Tuning, or the
``T`` below, which restates the derivation so that the oracle does not lean on the code under test; its ``spec`` is what an
options.Tuning is built from on the other side).  The margin is how far the
closest of all note decisions stood from going the other way: over every pitched frame the gap between the distances of the two
nearest allowed notes to the centre, and, wherever the candidate differs from the note held, | |c - cand| + HYST - |c - held| |.
A GPU test may compare notes exactly only on inputs whose margin is far above what an ulp in a logarithm can move
(tests/test_tune_cpu.py pins that for every case below).
"""
import math
from collections import namedtuple

import numpy as np

import pitch_oracle as P

LN2 = P.LN2
S = LN2 / 12.0
H = 5
HYST = 0.25
FRAME_MS = 20.0
TONICS = {"c": 0, "c#": 1, "db": 1, "d": 2, "d#": 3, "eb": 3, "e": 4, "f": 5, "f#": 6, "gb": 6, "g": 7, "g#": 8, "ab": 8, "a": 9,
          "a#": 10, "bb": 10, "b": 11}
SCALES = {"major": "101011010101", "minor": "101101011010", "harmonic_minor": "101101011001", "pentatonic": "101010010100",
          "minor_pentatonic": "100101010010", "blues": "100101110010"}

T_ = namedtuple("T_", "mask strength alpha log_ref spec", defaults=(None,))


def mask_of(scale):
    """The scale grammar of the issue, restated: 'chromatic', '<tonic>:<name>', '<tonic>:<twelve 0/1 from the tonic>'."""
    text = scale.lower()
    if text == "chromatic":
        return 0xFFF
    tonic, pattern = text.split(":")
    pattern = SCALES.get(pattern, pattern)
    assert len(pattern) == 12 and "1" in pattern
    return sum(1 << ((TONICS[tonic] + j) % 12) for j, ch in enumerate(pattern) if ch == "1")


def T(scale, strength=1.0, retune_ms=80.0, tuning_hz=440.0):
    """(mask, sigma, a, log_ref) of a scale, a strength, a retune time and a tuning frequency; ``spec``: those four, as given."""
    a = 1.0 if retune_ms == 0 else -math.expm1(-FRAME_MS / retune_ms)
    return T_(mask_of(scale), float(strength), a, math.log(tuning_hz), (scale, float(strength), float(retune_ms), float(tuning_hz)))


def near(mask, c):
    """-> (nearest allowed integer to c, the lower of two equally near; its distance; the distance of the runner-up)"""
    f = int(math.floor(c))
    ks = [k for k in range(f - 12, f + 14) if (mask >> (((k % 12) + 12) % 12)) & 1]
    d = [abs(np.float64(k) - c) for k in ks]
    order = sorted(range(len(ks)), key=lambda j: (d[j], ks[j]))
    return ks[order[0]], d[order[0]], d[order[1]]


def tune_one(x, t):
    """One segment -> (y float32, notes int32, margin)."""
    x = np.asarray(x, np.float32)
    y, notes, margin = x.copy(), np.full(x.size, -1, np.int32), np.inf
    if t is None or t.mask == 0 or t.strength == 0:
        return y, notes, margin
    sigma, a, log_ref = np.float64(t.strength), np.float64(t.alpha), np.float64(t.log_ref)
    with np.errstate(invalid="ignore"):
        pitched = (x > 0) & (x < np.inf)
    l = np.zeros(x.size, np.float64)
    l[pitched] = np.log(x[pitched].astype(np.float64))
    m = (l - log_ref) / S + 69.0
    i = 0
    while i < x.size:
        if not pitched[i]:
            i += 1
            continue
        b = i
        while i < x.size and pitched[i]:
            i += 1
        e = i                                             # the run [b, e)
        n_prev, g = None, None
        for j in range(b, e):
            w = np.sort(m[max(b, j - H):min(e - 1, j + H) + 1])
            c = w[(w.size - 1) // 2]
            cand, d0, d1 = near(t.mask, c)
            margin = min(margin, float(d1 - d0))
            if n_prev is None:
                n = cand
            else:
                held = abs(c - np.float64(n_prev))
                lhs = d0 + HYST
                if cand != n_prev:
                    margin = min(margin, float(abs(lhs - held)))
                n = cand if lhs < held else n_prev
            err = np.float64(n) - m[j]
            g = err if g is None else g + a * (err - g)
            y[j] = np.float32(np.exp(l[j] + (sigma * g) * S))
            notes[j] = n
            n_prev = n
    return y, notes, margin


def tune(f0, seg, tunings):
    """The stacked segments of ``seg`` (row offsets) -> (y, notes, smallest margin over all segments)."""
    f0 = np.asarray(f0, np.float32)
    assert len(tunings) == len(seg) - 1 and seg[-1] == f0.size
    ys, ns, margin = [], [], np.inf
    for s, t in enumerate(tunings):
        y, n, mg = tune_one(f0[seg[s]:seg[s + 1]], t)
        ys.append(y); ns.append(n); margin = min(margin, mg)
    return np.concatenate(ys), np.concatenate(ns), margin


def grid_hz(notes, tuning_hz=440.0):
    """The frequency of each note on the equal-tempered grid of ``tuning_hz``, fp64."""
    return tuning_hz * 2.0 ** ((np.asarray(notes, np.float64) - 69.0) / 12.0)


# ---------------------------------------------------------------- the f0 cases of the GPU tests, pinned by tests/test_tune_cpu.py
CUSTOM = "D:100101001010"           # a custom pattern: D F G Bb C
MASKS = ("chromatic", "C:major", "G:major", CUSTOM)
SETTINGS = ((1.0, 0.0), (1.0, 80.0), (0.6, 200.0))          # (strength, retune_ms)


def hz(semis, ref=440.0):
    return (ref * 2.0 ** ((np.asarray(semis, np.float64) - 69.0) / 12.0)).astype(np.float32)


def melody_cases():
    """name -> f0: the raw and the median-shifted sources of pitch_oracle.cases() (1237 / 777 / 301 frames: odd lengths, more than
    one block, random short runs)."""
    out = {}
    for name, (src, pool, _why) in P.cases().items():
        out[name] = src
        out[name + "-shifted"] = P.shift(src, P.lower_median_log(src), P.lower_median_log(pool), P.MEDIAN)[0]
    return out


def steps():
    """A stepwise melody with long runs: 36 notes of 25 frames, each 35 cents sharp with 5 cents of seeded noise, a 6-frame gap
    after every fourth note: 954 frames."""
    rng = np.random.default_rng(36)
    degrees = [0, 2, 4, 5, 7, 9, 11, 12, 11, 9, 7, 5, 4, 2, 0, 2, 4, 7, 12, 7, 4, 0, 5, 9, 5, 2, 7, 11, 7, 4, 0, 4, 7, 4, 2, 0]
    parts = []
    for k, d in enumerate(degrees):
        parts.append(hz(57 + d + 0.35 + 0.05 * rng.uniform(-1, 1, 25)))
        if k % 4 == 3:
            parts.append(np.zeros(6, np.float32))
    f = np.concatenate(parts)
    assert f.size == 954
    return f


def one_run():
    """A single pitched run of 1500 frames: a slow glide over an octave plus a 5.5 Hz vibrato of +-0.5 semitone.  (A glide crosses
    every decision boundary on its way; the start is one at which no frame lands within 1e-6 of one — 55.2 does, at 3e-7.)"""
    i = np.arange(1500)
    return hz(55.23 + 12.0 * i / 1500.0 + 0.5 * np.sin(2 * np.pi * 5.5 * i * 0.02))


def edges():
    """-> (f0 stacked, seg, tunings, what each segment is for): hand-made segments around every boundary of the specification."""
    mel = lambda n, base, seed: hz(base + 0.31 + 3.0 * np.sin(np.arange(n) * 0.07 + seed) + 0.04 * np.random.default_rng(seed).uniform(-1, 1, n))
    z = lambda n: np.zeros(n, np.float32)
    runs = np.concatenate([np.concatenate([mel(n, 60 + k, 10 + k), z(2)]) for k, n in enumerate((1, 2, H, H + 1, 2 * H + 1, 2 * H + 2, 40))])
    ends = np.concatenate([mel(7, 62, 20), z(9), mel(13, 65, 21)])                  # a run at frame 0 and one at the last frame
    a_end = np.concatenate([z(5), mel(30, 64.0, 22)])                               # ends pitched ...
    b_start = np.concatenate([hz(np.full(30, 67.3) + 0.02 * np.sin(np.arange(30))), z(4)])      # ... the next starts pitched, 3 semitones up
    odd = mel(60, 58, 23)
    odd[11], odd[25], odd[40] = np.float32("nan"), np.float32("inf"), np.float32(-220.0)
    segs = [
        (runs, T("chromatic", 1.0, 80.0), "runs of 1, 2, H, H+1, 2H+1, 2H+2 and 40 frames"),
        (ends, T("C:major", 1.0, 0.0), "a run at frame 0 and one at the last frame"),
        (a_end, T("G:major", 0.7, 120.0, 442.0), "ends pitched"),
        (b_start, T("G:major", 0.7, 120.0, 442.0), "starts pitched 3 semitones away"),
        (z(33), T("chromatic"), "all unvoiced"),
        (hz([61.4]), T("A:minor", 1.0, 0.0), "one pitched frame"),
        (z(1), T("A:minor"), "one unpitched frame"),
        (odd, T(CUSTOM, 0.5, 40.0, 432.0), "a NaN, a +inf and a negative frame inside a melody"),
        (mel(50, 63, 24), None, "off between on segments"),
        (mel(45, 66, 25), T("E:blues", 1.0, 200.0, 415.0), "a single-digit alpha, baroque pitch"),
        (mel(41, 59, 26), T("C:100000000000", 0.9, 20.0), "a single pitch class"),
    ]
    f0 = np.concatenate([s[0] for s in segs])
    seg = [0]
    for s in segs:
        seg.append(seg[-1] + s[0].size)
    return f0, seg, [s[1] for s in segs], [s[2] for s in segs]


def kernel_cases():
    """name -> (f0, seg, tunings): every oracle comparison the GPU child makes on the kernel, so that tests/test_tune_cpu.py can
    pin the margin of each without a GPU."""
    out = {}
    f0, seg, tun, _ = edges()
    out["edges"] = (f0, seg, tun)
    combos = [T(mk, st, ms) for mk in MASKS for st, ms in SETTINGS]
    for name, src in melody_cases().items():
        out[name] = (np.tile(src, len(combos)), [k * src.size for k in range(len(combos) + 1)], combos)
    extra = combos + [T("C:100000000000", 1.0, 80.0)]
    for name, src in (("steps", steps()), ("one-run", one_run())):
        out[name] = (np.tile(src, len(extra)), [k * src.size for k in range(len(extra) + 1)], extra)
    return out
