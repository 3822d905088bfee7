"""What the two output-dynamics stages cost beside the generator they follow: ops.envelope_mix and ops.limit_peak on 480 000
samples (30 s) against Vocoder.forward (hipGraph replay) of the same 1500 frames with the full-size `mix` generator.  HIP events,
same process, the stages alternating; writes the kernel-timing part of profiles/dynamics.txt (or the path given).

    python tools/dynamics_tail.py [OUT.txt] [REPS]

The ceiling is timed three ways: on the generator's own output with a ceiling above its peak (every tile takes the all-ones
shortcut), with a ceiling at half its peak (the common case: some tiles engage), and with a ceiling under nearly every sample
(every tile runs the window minimum and the 2L + 1-tap sum); and once in place (one workgroup walks the tiles in order)."""
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import dynamics_oracle as O
from knn_svc_amd import config as C, ops, synthetic as S
from knn_svc_amd.vocoder import Vocoder

out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "dynamics.txt")
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 200
dev, N = "cuda", 1500
torch.cuda.set_device(0)
gen = torch.Generator().manual_seed(0)
voc = Vocoder(S.seeded_state(S.generator_param_spec(C.HIFIGAN_V1, "mix"), seed=2), C.HIFIGAN_V1, "mix", dev)
c = (0.3 * torch.randn(N, 1024, generator=gen)).to(dev)
f0 = (150 + 100 * torch.rand(N, generator=gen)).to(dev)
harm = (0.02 * torch.rand(N, 49, generator=gen)).to(dev)
src = torch.from_numpy(O.phrased(N, 3)).to(dev)
ev = lambda: torch.cuda.Event(enable_timing=True)
with torch.inference_mode():
    for _ in range(5):                       # eager at first sight, captured at the second, replayed from then on
        y = voc.forward(c, f0, harm)
    y = y.clone()
    peak = float(y.abs().max())
    db = lambda v: min(0.0, 20 * math.log10(v))
    stages = {
        "envelope_mix (3 launches, in place)": lambda: ops.envelope_mix(y, src, 0.7, out=work),
        "limit_peak, ceiling above the peak (all tiles copy)": lambda: ops.limit_peak(work, db(min(1.0, 1.01 * peak)), out=out),
        "limit_peak, ceiling at half the peak": lambda: ops.limit_peak(work, db(0.5 * peak), out=out),
        "limit_peak, ceiling at 1e-3 of the peak (every tile engages)": lambda: ops.limit_peak(work, db(1e-3 * peak), out=out),
        "limit_peak, ceiling at half the peak, IN PLACE (one workgroup)": lambda: ops.limit_peak(work, db(0.5 * peak), out=work),
    }
    work, out = y.clone(), torch.empty_like(y)
    engaged = {}
    for name, fn in stages.items():
        for _ in range(5):
            work.copy_(y)
            fn()
    for name in list(stages)[1:4]:
        work.copy_(y)
        p = {"above": db(min(1.0, 1.01 * peak)), "half the peak": db(0.5 * peak), "1e-3": db(1e-3 * peak)}
        key = next(k for k in p if k in name)
        engaged[name] = int(ops.limit_peak(work, p[key], return_stats=True)[1][0])
    torch.cuda.synchronize()
    times = {name: [] for name in stages}
    t_gen = []
    for _ in range(reps):
        a, b = ev(), ev()
        a.record()
        voc.forward(c, f0, harm)
        b.record()
        marks = []
        for name, fn in stages.items():
            work.copy_(y)
            s, e = ev(), ev()
            s.record()
            fn()
            e.record()
            marks.append((name, s, e))
        torch.cuda.synchronize()
        t_gen.append(a.elapsed_time(b))
        for name, s, e in marks:
            times[name].append(s.elapsed_time(e))
q = lambda v: (float(np.min(v)), float(np.median(v)), float(np.percentile(v, 90)))
g = q(t_gen)
lines = [f"output dynamics beside the generator, 1 x {torch.cuda.get_device_name(0)}, {N} frames = {N * 320} samples, {reps} repetitions after 5 warm-up",
         "calls each, the stages alternating in one process, HIP events (each figure includes the host's enqueue of its launches)",
         f"generator output peak {peak:.4f}",
         f"{'stage':<66} {'min ms':>8} {'median':>8} {'90th':>8}   share of the generator (medians)",
         f"{'Vocoder.forward (full-size mix generator, hipGraph replay + copy out)':<66} {g[0]:8.3f} {g[1]:8.3f} {g[2]:8.3f}"]
for name, v in times.items():
    t = q(v)
    extra = f"   limited samples {engaged[name]}" if name in engaged else ""
    lines.append(f"{name:<66} {t[0]:8.3f} {t[1]:8.3f} {t[2]:8.3f}   {t[1] / g[1]:.3f}{extra}")
text = "\n".join(lines) + "\n"
print(text)
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
open(out_path, "w").write(text)
