"""Match stage by neighbours per frame: time of matching.match_features with the neighbour lists given (no search), events
around each call, at the bench's point — 1500 query frames, a 30 000-frame pool, dim 1024, "mix", post_opt_0.2 — for
topk = 1, 2, 4, 8 and for 4 without its fast paths (KNNSVC_MATCH_GENERIC_K=1).

    python tools/topk_ab.py [--reps 9] [--out profiles/topk_match_stage.txt]

Per row: median / min / max of the repetitions after three warm-up calls, and the iteration counts of the two Adam loops (the
time of the stage follows them).  Temporally smooth synthetic features, as tools/match_bench.py."""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from knn_svc_amd import config as C, matching as M, synthetic as S

KNOB = "KNNSVC_MATCH_GENERIC_K"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = "cuda"
    nq, npool = 1500, 30000
    sm = lambda x: (x + torch.roll(x, 1, 0) + torch.roll(x, 2, 0)) / 3
    q = sm(S.clustered_features(nq, 1024, 1, n_centres=60)).to(dev)
    p = sm(S.clustered_features(npool, 1024, 2, n_centres=60)).to(dev)
    _, f0 = S.synth_clip(npool * 320, 3); pf0 = torch.from_numpy(f0[:npool].copy()).to(dev)
    _, f0 = S.synth_clip(nq * 320, 4); qf0 = torch.from_numpy(f0[:nq].copy() * 1.2).to(dev)
    harm = (torch.rand(npool, 49, generator=torch.Generator().manual_seed(5)) * 0.05).to(dev)
    prep = M.prepare_pool(p)
    nn32, _fl = M.batched_knn(q, p, prep)
    lines = [f"match stage (match_features, nn32 given): {nq} query frames, {npool}-frame pool, dim 1024, mix / post_opt_0.2, "
             f"{a.reps} repetitions after 3 warm-up calls, {torch.cuda.get_device_name(0)}",
             f"{'topk':<12}{'median ms':>11}{'min ms':>9}{'max ms':>9}   Adam iterations (WavLM / harmonics)"]
    for k, generic in ((1, False), (2, False), (4, False), (4, True), (8, False)):
        if generic:
            os.environ[KNOB] = "1"
        try:
            run = lambda: M.match_features(q, qf0, p, pf0, harm, "mix", "post_opt_0.2", return_debug=True, nn32=nn32, pool_prep=prep, topk=k)
            for _ in range(3):
                out = run()
            ts = []
            for _ in range(a.reps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize(); e0.record()
                out = run()
                e1.record(); torch.cuda.synchronize()
                ts.append(e0.elapsed_time(e1))
        finally:
            os.environ.pop(KNOB, None)
        assert out[3]["idx_wavlm"].shape == (nq, k) and bool(torch.isfinite(out[0]).all())
        lines.append(f"{str(k) + (' generic' if generic else ''):<12}{statistics.median(ts):>11.3f}{min(ts):>9.3f}{max(ts):>9.3f}   "
                     f"{int(out[3]['iters_wavlm'])} / {int(out[3]['iters_harm'])}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
