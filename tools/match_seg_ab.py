"""A/B of the match-stage routes of serving.BatchConverter on one box, in one process: match="lanes" (one match body per source on
three lane streams) against match="segmented" (the sources of a batch stacked, one workgroup per source in every recurrence
launch), swept over match_batch.  Seeded full-size models (the ones bench.py uses), sources resident in HBM.

  workload a   32 x 30 s sources against a 60-minute resident pool (bench.py's cfg-5 share)
  workload b   64 x 3 s sources against a 10-minute pool

    python tools/match_seg_ab.py [--workload a|b|ab] [--warmup 2] [--rounds 5] [--batches 4,8,16,32,64] [--out FILE]

Per configuration: ms per source (median and min..max of the timed rounds; host clock around convert() + a device sync, i.e. from
the first launch to the last waveform of the batch) and that batch time itself.  The configurations are visited in the same order
in every round (lanes, then the sweep), so a drift of the box shows up in all of them alike; the first `--warmup` rounds (first
sight runs eagerly, the second captures the graphs) are not timed."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from knn_svc_amd import config as C, serving, synthetic as S
from knn_svc_amd.matcher import KNeighborsVC
from knn_svc_amd.vocoder import Vocoder
from knn_svc_amd.wavlm import WavLMEncoder

WORKLOADS = {"a": dict(sources=32, src_s=30, pool_clips=120, clip_s=30, what="32 x 30 s sources vs a 60-minute pool"),
             "b": dict(sources=64, src_s=3, pool_clips=20, clip_s=30, what="64 x 3 s sources vs a 10-minute pool")}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="ab")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--batches", default="4,8,16,32,64")
    ap.add_argument("--out", default=None, help="append the table to this file as well")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    enc = WavLMEncoder(S.seeded_state(S.wavlm_param_spec(C.WAVLM_LARGE, 6), seed=1), C.WAVLM_LARGE, dev, 6)
    voc = Vocoder(S.seeded_state(S.generator_param_spec(C.HIFIGAN_V1, "mix"), seed=2), C.HIFIGAN_V1, "mix", dev)
    vc = KNeighborsVC(enc, voc, C.HIFIGAN_V1, dev)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    with torch.inference_mode():
        for key in a.workload:
            wl = WORKLOADS[key]
            tv = serving.TargetVoice.from_clips(vc, [S.synth_clip(wl["clip_s"] * C.SAMPLE_RATE, seed=5000 + i) for i in range(wl["pool_clips"])])
            reqs = [(torch.from_numpy(w).to(dev), torch.from_numpy((f * 1.3).astype(np.float32)).to(dev))
                    for w, f in (S.synth_clip(wl["src_s"] * C.SAMPLE_RATE, seed=7000 + i) for i in range(wl["sources"]))]
            confs = [("lanes", None)] + [("segmented", int(b)) for b in a.batches.split(",") if int(b) <= max(4, wl["sources"])]
            convs = [serving.BatchConverter(vc, tv, "mix", "post_opt_0.2", match=m, match_batch=b) for m, b in confs]
            times = [[] for _ in confs]
            ref = None
            for rnd in range(a.warmup + a.rounds):
                for k, conv in enumerate(convs):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    ys = conv.convert(reqs)
                    torch.cuda.synchronize()
                    dt = time.perf_counter() - t0
                    if rnd >= a.warmup:
                        times[k].append(dt)
                    if rnd == a.warmup:               # the routes must agree sample for sample
                        if ref is None:
                            ref = [y.clone() for y in ys]
                        elif not all(torch.equal(x, y) for x, y in zip(ref, ys)):
                            say(f"# WARNING: {confs[k]} differs from lanes")
            say(f"# workload {key}: {wl['what']} ({tv.frames} pool frames), {a.rounds} timed rounds after {a.warmup} warm-up rounds")
            say(f"# {'route':<22}{'ms/source median':>18}{'min':>9}{'max':>9}{'batch ms median':>18}")
            for (m, b), ts in zip(confs, times):
                per = [t / wl["sources"] * 1e3 for t in ts]
                name = m if b is None else f"{m} batch={b}"
                say(f"  {name:<22}{statistics.median(per):>18.3f}{min(per):>9.3f}{max(per):>9.3f}{statistics.median(ts) * 1e3:>18.1f}")
            say(json.dumps({"workload": key, "rows": [{"match": m, "match_batch": b, "ms_per_source": [round(t / wl["sources"] * 1e3, 3) for t in ts]}
                                                      for (m, b), ts in zip(confs, times)]}))
            del tv, reqs, convs, ref
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
