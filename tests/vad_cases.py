"""The seeded 16 kHz inputs of the trimmer's tests (a helper: no test in here), shared by tests/test_vad_cpu.py (which shows, on
the oracle alone, that no decision of any case stands closer than MARGIN to flipping) and tests/test_gpu_vad.py (which runs the
same cases on the device).  CASES: name -> (waveform float32, trigger level)."""
import os

import numpy as np

SR = 16000
MARGIN = 1e-6
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def noise(n, seed, amp=1e-3):
    return amp * np.random.default_rng(seed).standard_normal(n)


def voiced(n, f_from=180.0, f_to=260.0, amp=0.2, harmonics=12):
    """A gliding harmonic tone (amplitudes 1/h) with a 10 ms fade at both ends."""
    t = np.arange(n) / SR
    f0 = f_from + (f_to - f_from) * t / max(t[-1], 1e-9)
    phase = 2 * np.pi * np.cumsum(f0) / SR
    y = sum(np.sin(h * phase) / h for h in range(1, harmonics + 1))
    fade = np.minimum(1.0, np.minimum(np.arange(n), np.arange(n)[::-1]) / 160.0)
    return amp * fade * y


def tone(n, f=220.0, amp=0.2, harmonics=8):
    t = np.arange(n) / SR
    return amp * sum(np.sin(2 * np.pi * f * h * t) / h for h in range(1, harmonics + 1))


def place(total, seed, *parts):
    """Faint noise of ``total`` samples with (start sample, signal) parts added."""
    x = noise(total, seed)
    for at, sig in parts:
        x[at:at + sig.size] += sig
    return x.astype(np.float32)


def short(n, seed):
    """Shorter than the boot phase: M = 0, 1, 1, 2 measurements at 1599, 1600, 2399, 2400 samples; never triggers."""
    return place(n, seed, (0, tone(n)))


def tone2s(seed=21):
    """2 s: 0.6 s of 1e-3 noise, then a 220 Hz tone with harmonics until 1.5 s (more than 7 measurements: the boot phase ends and
    the steady state triggers), noise again behind it so that the reversed pass has a noise floor to start from."""
    return place(2 * SR, seed, (9600, tone(14400)))


def early_burst(seed=22):
    """Speech from 0.2 s on, inside the boot phase (its six measurements end at 0.35 s): the walk-back runs into the boot's
    zero measures and to the start of the recording."""
    return place(int(1.8 * SR), seed, (3200, voiced(int(1.0 * SR))))


def two_bursts(gap_measurements, seed=23):
    """A 60 ms burst (too short to fire on its own), silence, then 0.6 s of speech.  The silence is sized so that
    ``gap_measurements`` measurements between the two stand clear of both (3: within gap_len = 5, the walk-back reaches over
    to the first burst; 8: beyond it, the cut lands in front of the second)."""
    a, b = voiced(960, 200.0, 230.0), voiced(9600)
    first = 9600
    second = first + a.size + 1600 + gap_measurements * 800
    return place(second + b.size + 9600, seed, (first, a), (second, b))


def short_voiced(seed=24):
    """0.3 s of speech between 0.5 s of noise on either side: the front cut shortens what the reversed scan may use."""
    return place(int(1.3 * SR), seed, (8000, voiced(4800)))


def tone_8k(seed=25):
    """The 2 s case at 8 kHz (measurements of 800 samples every 400, 1024-point transform, 506 bins, 24 cepstrum bins): the
    constants that follow the rate.  -> (waveform, level, rate)"""
    sr = 8000
    t = np.arange(int(0.9 * sr)) / sr
    x = noise(2 * sr, seed)
    x[int(0.6 * sr):int(0.6 * sr) + t.size] += 0.2 * sum(np.sin(2 * np.pi * 220.0 * h * t) / h for h in range(1, 9))
    return x.astype(np.float32), 7.0, sr


def golden_target():
    import sys
    sys.path.insert(0, ROOT)
    from knn_svc_amd import audio_io
    x, sr = audio_io.read_wav(os.path.join(ROOT, "tests", "golden", "sample_content", "tgt.wav"))
    assert sr == SR
    return np.ascontiguousarray(x[0], dtype=np.float32)


def cases():
    c = {f"n{n}": (short(n, 30 + i), 7.0) for i, n in enumerate((1599, 1600, 2399, 2400))}
    c["tone2s/3"] = (tone2s(), 3.0)
    c["tone2s/7"] = (tone2s(), 7.0)
    c["tone2s/12"] = (tone2s(), 12.0)
    c["early-burst"] = (early_burst(), 7.0)
    c["two-bursts/gap3"] = (two_bursts(3), 7.0)
    c["two-bursts/gap8"] = (two_bursts(8), 7.0)
    c["short-voiced"] = (short_voiced(), 7.0)
    c["golden-tgt"] = (golden_target(), 7.0)
    return c
