"""What trimming a pool costs: ops.vad_trim (knnsvc_vad_trim_seg: tables, spectrum, track, cepstrum, trigger) ONCE over a synthetic
600 s pool of 20 x 30 s recordings (the pool of bench.py's step), HIP events around the call, and the same pool one recording per
call (what matching.get_complete_spk_pool does).  Writes profiles/vad_trim.txt of this repository (or the path given).

    python tools/vad_bench.py [OUT.txt] [REPS]"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from knn_svc_amd import ops

out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "vad_trim.txt")
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 20
dev, files, secs, sr = "cuda", 20, 30, 16000
torch.cuda.set_device(0)


def recording(seed):
    """1 s of faint noise, 28 s of a gliding harmonic tone under a syllable-rate envelope, 1 s of faint noise."""
    rng = np.random.default_rng(seed)
    n = secs * sr
    x = 1e-3 * rng.standard_normal(n)
    t = np.arange(n - 2 * sr) / sr
    phase = 2 * np.pi * np.cumsum(140.0 + 60.0 * np.sin(2 * np.pi * 0.3 * t + seed)) / sr
    env = 0.15 * (0.55 + 0.45 * np.sin(2 * np.pi * 3.1 * t))
    x[sr:n - sr] += env * sum(np.sin(h * phase) / h for h in range(1, 11))
    return torch.from_numpy(x.astype(np.float32)).to(dev)


wavs = [recording(s) for s in range(files)]
ev = lambda: torch.cuda.Event(enable_timing=True)
with torch.inference_mode():
    for _ in range(3):
        strip = ops.vad_trim(wavs, 7.0)
        for w in wavs[:2]:
            ops.vad_trim(w, 7.0)
    torch.cuda.synchronize()
    t_all, t_each = [], []
    for _ in range(reps):
        a, b, c = ev(), ev(), ev()
        a.record()
        strip = ops.vad_trim(wavs, 7.0)
        b.record()
        for w in wavs:
            ops.vad_trim(w, 7.0)
        c.record()
        torch.cuda.synchronize()
        t_all.append(a.elapsed_time(b)); t_each.append(b.elapsed_time(c))
kept = strip.cpu().numpy()
q = lambda v: (float(np.median(v)), float(np.percentile(v, 10)), float(np.percentile(v, 90)))
one, each = q(t_all), q(t_each)
dropped = int((kept[:, 0] < 0).sum())
cut = float(kept[kept[:, 0] >= 0].sum()) / sr
text = (f"pool-silence trimming, 1 x MI355X, {files} x {secs} s = {files * secs} s at {sr} Hz, level 7, {reps} repetitions, HIP events\n"
        f"(each figure includes the host's enqueue, the concatenation of the recordings and the workspace allocation; median [10th .. 90th percentile])\n"
        f"ops.vad_trim, all {files} recordings in one call (5 launches): {one[0]:.3f} ms [{one[1]:.3f} .. {one[2]:.3f}]\n"
        f"ops.vad_trim, one call per recording ({5 * files} launches):     {each[0]:.3f} ms [{each[1]:.3f} .. {each[2]:.3f}]\n"
        f"recordings dropped: {dropped}; trimmed away in total: {cut:.2f} s\n")
print(text)
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
open(out_path, "w").write(text)
