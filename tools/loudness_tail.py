"""What the loudness tail costs beside the generator it follows: knnsvc_loudness + knnsvc_loudness_gain on 480 000 samples against
Vocoder.forward (hipGraph replay) of the same 1500 frames with the full-size `mix` generator.  HIP events, same process, the two
alternating; writes profiles/loudness_tail.txt of this repository (or the path given).

    python tools/loudness_tail.py [OUT.txt] [REPS]"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from knn_svc_amd import config as C, ops, synthetic as S
from knn_svc_amd.vocoder import Vocoder

out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "loudness_tail.txt")
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 200
dev, N = "cuda", 1500
torch.cuda.set_device(0)
gen = torch.Generator().manual_seed(0)
voc = Vocoder(S.seeded_state(S.generator_param_spec(C.HIFIGAN_V1, "mix"), seed=2), C.HIFIGAN_V1, "mix", dev)
c = (0.3 * torch.randn(N, 1024, generator=gen)).to(dev)
f0 = (150 + 100 * torch.rand(N, generator=gen)).to(dev)
harm = (0.02 * torch.rand(N, 49, generator=gen)).to(dev)
with torch.inference_mode():
    for _ in range(5):                       # eager at first sight, captured at the second, replayed from then on
        y = voc.forward(c, f0, harm)
    for _ in range(5):
        ops.normalize_loudness(y.clone(), -16.0)
    torch.cuda.synchronize()
    ev = lambda: torch.cuda.Event(enable_timing=True)
    t_gen, t_ld = [], []
    for _ in range(reps):
        a, b, d = ev(), ev(), ev()
        a.record()
        y = voc.forward(c, f0, harm)
        b.record()
        ops.normalize_loudness(y, -16.0, out=y)
        d.record()
        torch.cuda.synchronize()
        t_gen.append(a.elapsed_time(b)); t_ld.append(b.elapsed_time(d))
    lk = float(ops.loudness(voc.forward(c, f0, harm)))
q = lambda v: (float(np.median(v)), float(np.percentile(v, 10)), float(np.percentile(v, 90)))
g, l = q(t_gen), q(t_ld)
text = (f"loudness tail beside the generator, 1 x MI355X, {N} frames = {N * 320} samples, {reps} alternating repetitions, HIP events\n"
        f"(each figure includes the host's enqueue of its launches; median [10th .. 90th percentile])\n"
        f"Vocoder.forward (full-size mix generator, hipGraph replay + copy out): {g[0]:.3f} ms [{g[1]:.3f} .. {g[2]:.3f}]\n"
        f"knnsvc_loudness + knnsvc_loudness_gain (5 launches, in place):          {l[0]:.3f} ms [{l[1]:.3f} .. {l[2]:.3f}]\n"
        f"ratio tail / generator: {l[0] / g[0]:.3f}\n"
        f"loudness of the seeded generator's output: {lk:.3f} LKFS\n")
print(text)
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
open(out_path, "w").write(text)
