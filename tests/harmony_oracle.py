"""numpy restatement of the section "Harmony voice" of include/knnsvc_hip.h: the reference for knnsvc_harmony_f0_seg, and of
knnsvc_mix_waves.  fp64 everywhere, every step rounded on its own (numpy never contracts), the output rounded once to fp32.
Steps 1 to 4 (pitched frames, semitones, centre, note with hysteresis) are tests/tune_oracle.py's: the specification says they
are "Pitch correction"'s word for word.  The lead's f0 is an INPUT: the GPU tests feed the device's own.

    harmony(f0, seg, parts) -> (part f0 float32, part notes t int32 (-1: unpitched), D = t - n int32 (0: unpitched),
                                pitched bool, smallest decision margin in semitones)

``parts``: per segment None (off) or anything with ``mask`` / ``steps`` / ``alpha`` / ``log_ref`` (options.HarmonyShift, or the
``P`` below, which restates the derivation and carries the ``scale`` / ``tuning_hz`` it was built from).  The margin is
tune_oracle's: how far the closest note decision of steps 3 and 4 stood from going the other way; everything behind the note is
integer arithmetic and a contraction.
"""
import math
from collections import namedtuple

import numpy as np

import tune_oracle as O

S = O.S
P_ = namedtuple("P_", "mask steps alpha log_ref scale tuning_hz glide_ms", defaults=(None, 440.0, None))
MAX_STEPS = 24


def P(scale, steps, glide_ms=40.0, tuning_hz=440.0):
    """(mask, steps, a, log_ref) of a scale, a number of degrees, a glide time and a tuning frequency."""
    a = 1.0 if glide_ms == 0 else -math.expm1(-O.FRAME_MS / glide_ms)
    return P_(O.mask_of(scale), int(steps), a, math.log(tuning_hz), scale, float(tuning_hz), float(glide_ms))


def degrees(mask):
    """The allowed pitch classes, ascending."""
    return [k for k in range(12) if (mask >> k) & 1]


def degree_move(mask, n, steps):
    """Step 5: the allowed note ``n`` moved by ``steps`` degrees -> (t, floordiv(J, d)).  Python's // and % are the floor
    division and the non-negative remainder the specification asks for."""
    pcs = degrees(mask)
    d = len(pcs)
    pc = n % 12
    j = pcs.index(pc)                                  # n is allowed by construction
    o = (n - pc) // 12
    J = j + steps
    return 12 * (o + J // d) + pcs[J % d], J // d


_NOTES = {}


def lead_notes(x, mask, log_ref):
    """Steps 1 to 4 through tune_oracle (strength and retune do not enter the note) -> (notes, margin); kept per input, since
    the GPU cases stack one source under many settings."""
    key = (x.tobytes(), int(mask), float(log_ref))
    if key not in _NOTES:
        _y, n, margin = O.tune_one(x, O.T_(mask, 1.0, 1.0, log_ref))
        _NOTES[key] = (n, margin)
    return _NOTES[key]


def harmony_one(x, p):
    """One segment -> (y float32, t int32, D int32, pitched, margin, octave carries seen: a set of floordiv(J, d) values)."""
    x = np.asarray(x, np.float32)
    with np.errstate(invalid="ignore"):
        pitched = (x > 0) & (x < np.inf)
    y, t, D = x.copy(), np.full(x.size, -1, np.int32), np.zeros(x.size, np.int32)
    if p is None or p.mask == 0 or p.steps == 0:
        return y, t, D, np.zeros(x.size, bool), np.inf, set()
    n, margin = lead_notes(x, p.mask, p.log_ref)
    a = np.float64(p.alpha)
    l = np.zeros(x.size, np.float64)
    l[pitched] = np.log(x[pitched].astype(np.float64))
    carries = set()
    moved = {}
    h = None
    for i in range(x.size):
        if not pitched[i]:
            h = None                                   # a run ends
            continue
        ni = int(n[i])
        if ni not in moved:
            moved[ni] = degree_move(p.mask, ni, p.steps)
        ti, q = moved[ni]
        carries.add(q)
        Di = np.float64(ti - ni)
        h = Di if h is None else h + a * (Di - h)
        y[i] = np.float32(np.exp(l[i] + h * S))
        t[i], D[i] = ti, ti - ni
    return y, t, D, pitched, margin, carries


def harmony(f0, seg, parts):
    f0 = np.asarray(f0, np.float32)
    assert len(parts) == len(seg) - 1 and seg[-1] == f0.size
    out = [harmony_one(f0[seg[s]:seg[s + 1]], p) for s, p in enumerate(parts)]
    cat = lambda k: np.concatenate([o[k] for o in out])
    return cat(0), cat(1), cat(2), cat(3), min(o[4] for o in out)


def parallel(f0, steps):
    """The oracle-free identity of the chromatic mask: every pitched frame times 2^(steps / 12), as the specification writes
    it -> fp32; the other frames as they are."""
    x = np.asarray(f0, np.float32)
    with np.errstate(invalid="ignore"):
        pitched = (x > 0) & (x < np.inf)
    y = x.copy()
    y[pitched] = np.exp(np.log(x[pitched].astype(np.float64)) + np.float64(steps) * S).astype(np.float32)
    return y


def mix(ys, gains):
    """knnsvc_mix_waves: (float)(sum_v g_v * (double)y_v) over the voices with a non-zero gain, in order, the sum starting with
    the first product."""
    acc = None
    for y, g in zip(ys, gains):
        if g == 0.0:
            continue
        p = np.float64(g) * np.asarray(y, np.float32).astype(np.float64)
        acc = p if acc is None else acc + p
    return acc.astype(np.float32)


# ---------------------------------------------------------------- the f0 cases of the GPU tests, pinned by tests/test_harmony_cpu.py
MASKS = ("C:100000000000", O.CUSTOM, "G:major", "chromatic")          # d = 1, 5, 7, 12
GLIDES = (0.0, 40.0, 189.8)                                           # a = 1, 0.39, 0.1
assert [round(P("chromatic", 1, g).alpha, 2) for g in GLIDES] == [1.0, 0.39, 0.1]


def step_set(scale):
    d = len(degrees(O.mask_of(scale)))
    return [1, -1, 2, -2, d, -d, MAX_STEPS, -MAX_STEPS]


def low():
    """A stepwise melody around and below 8.18 Hz (note 0 at 440): notes -15 .. 4, each 12 frames 35 cents sharp with seeded
    noise, a rest after every fifth: negative notes, and notes whose pitch class index wraps below zero."""
    rng = np.random.default_rng(81)
    notes = [4, 2, 0, -1, -3, -5, -7, -8, -10, -12, -13, -15, -12, -8, -5, -1, 2, -3, -10, 0]
    parts = []
    for k, nt in enumerate(notes):
        parts.append(O.hz(nt + 0.35 + 0.05 * rng.uniform(-1, 1, 12)))
        if k % 5 == 4:
            parts.append(np.zeros(3, np.float32))
    return np.concatenate(parts)


def edges():
    """tune_oracle.edges() (runs of 1, 2, H, H+1, 2H+1, 2H+2 and 40 frames; NaN, inf and negative frames; an off segment between
    on ones; adjacent pitched segment ends; its masks, among them d = 1, 5, 6, 7 and 12, and tuning frequencies) with a part
    per segment, and one more segment whose mask is on and whose steps are 0: off as well."""
    f0, seg, tun, why = O.edges()
    steps = [2, -2, 1, -1, 3, 5, -5, 2, None, -3, 1]
    glides = [40.0, 0.0, 189.8, 189.8, 40.0, 0.0, 40.0, 40.0, None, 189.8, 40.0]
    parts = [None if t is None else P(t.spec[0], s, g, t.spec[3]) for t, s, g in zip(tun, steps, glides)]
    extra = O.hz(60.3 + np.sin(np.arange(37) * 0.2))
    return (np.concatenate([f0, extra]), seg + [seg[-1] + extra.size], parts + [P("C:major", 0)],
            why + ["a scale and steps = 0: off"])


def stack(src, parts):
    return np.tile(src, len(parts)), [k * src.size for k in range(len(parts) + 1)], parts


def kernel_cases():
    """name -> (f0, seg, parts): every oracle comparison the GPU child makes on the kernel."""
    out = {}
    f0, seg, parts, _ = edges()
    out["edges"] = (f0, seg, parts)
    # the stepwise melody (a note change every 25 frames) under every mask, step and glide: 96 segments, two library calls
    out["steps"] = stack(O.steps(), [P(m, s, g) for m in MASKS for s in step_set(m) for g in GLIDES])
    out["one-run"] = stack(O.one_run(), [P(m, s, 40.0) for m in MASKS for s in step_set(m)[:6]])
    out["low"] = stack(low(), [P(m, s, 40.0) for m in MASKS for s in step_set(m)])
    return out
