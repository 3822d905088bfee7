"""numpy restatement of the pitch-control table in include/knnsvc_hip.h ("Pitch control"): the reference for
knnsvc_shift_f0_seg_mode.  fp32 where the table says fp32, fp64 where it says fp64, every step rounded on its own (numpy never
contracts).  The medians are INPUTS: the GPU tests feed the device's own, so what is compared is the shift, not the radix select.

    shift(f0, qm, pm, mode, t) -> (shifted f0 float32, applied interval in semitones float32)
"""
import numpy as np

MEDIAN, OCTAVE, SEMITONE, NONE = range(4)
MODES = {"median": MEDIAN, "octave": OCTAVE, "semitone": SEMITONE, "none": NONE}
LN2 = float(np.log(np.float64(2.0)))          # fp64 ln 2 = 0x1.62e42fefa39efp-1
S = LN2 / 12.0
TRANSPOSE_MAX = 36.0
assert LN2.hex() == "0x1.62e42fefa39efp-1"


def log_rn(f):
    """fp32 log evaluated in fp64 and rounded once."""
    return np.log(np.asarray(f, np.float32).astype(np.float64)).astype(np.float32)


def exp_rn(v):
    return np.exp(np.asarray(v, np.float32).astype(np.float64)).astype(np.float32)


def lower_median_log(f0):
    """torch.median (lower median) of log_rn over the voiced frames, NaN without one: what log_f0_median[_seg] returns."""
    v = np.sort(log_rn(f0[f0 != 0]))
    return np.float32(v[(v.size - 1) // 2]) if v.size else np.float32("nan")


def interval(qm, pm, mode, t):
    """-> (fp32 addend to log f0 for octave / semitone / none — for median the addend of the TRANSPOSE only —, fp32 applied
    interval in semitones)."""
    t = np.float32(t)
    ts = np.float64(t) * S
    if mode == NONE:
        return np.float32(ts), t
    with np.errstate(invalid="ignore"):
        d = np.float64(np.float32(pm)) - np.float64(np.float32(qm))
        if mode == MEDIAN:
            return np.float32(ts), np.float32(d / S + np.float64(t))
        step = LN2 if mode == OCTAVE else S
        q = step * np.rint(d / step) + ts          # np.rint: half to even
        return np.float32(q), np.float32(q / S)


def shift(f0, qm, pm, mode, t=0.0):
    f0 = np.asarray(f0, np.float32)
    add, semis = interval(qm, pm, mode, t)
    out = f0.copy()                                # unvoiced frames: the input's bits
    voiced = f0 != 0
    L = log_rn(f0[voiced])
    with np.errstate(invalid="ignore"):
        if mode == MEDIAN:
            v = (L + np.float32(pm)).astype(np.float32) - np.float32(qm)
            if np.float32(t) != 0:
                v = v + add
        else:
            v = L + add
        out[voiced] = exp_rn(v.astype(np.float32))
    return out, semis


def tie_distance(qm, pm):
    """How far d / LN2 and d / S stand from a rounding tie (x.5): (octave, semitone)."""
    d = np.float64(np.float32(pm)) - np.float64(np.float32(qm))
    far = lambda x: float(abs((x - np.floor(x)) - 0.5))
    return far(d / LN2), far(d / S)


# ---------------------------------------------------------------- the f0 cases of the GPU tests, pinned by tests/test_pitch_cpu.py
def track(n, base_hz, seed, voiced=0.7):
    """A synthetic f0 track: a slow melody around ``base_hz`` (+-4 semitones), unvoiced stretches as exact zeros."""
    rng = np.random.default_rng(seed)
    semis = 4.0 * np.sin(np.arange(n) * 0.013 + rng.uniform(0, 6)) + 0.3 * rng.standard_normal(n)
    f = (base_hz * 2.0 ** (semis / 12.0)).astype(np.float32)
    f[rng.uniform(size=n) > voiced] = 0.0
    return f


def cases():
    """name -> (source f0, pool f0, what the case is for).  Lengths: odd, no multiple of the 256-thread block, more than one block."""
    return {
        "up": (track(1237, 110.0, 1), track(2011, 233.0, 2), "octave -> +1 (d ~ +13 semitones)"),
        "down": (track(777, 392.0, 3), track(1500, 185.0, 4), "octave -> -1 (d ~ -13 semitones)"),
        "near": (track(301, 200.0, 5), track(900, 246.0, 6), "octave -> 0, semitone -> +4 or so"),
    }
