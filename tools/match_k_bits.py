"""Match stage, bit identity across builds: one crc32 per case of the walk's output and of the smoothness weights and iteration
counts, for k = 1, 3, 4, 8 and for k = 4 on the generic route (KNNSVC_MATCH_GENERIC_K=1).  Run it on two builds
(KNNSVC_LIB=/path/to/the/other/libknnsvc_hip.so selects one) and compare the outputs line by line.

    python tools/match_k_bits.py [--out FILE]

Walk: segments of 3 and 127 frames on a 4000-row pool, dims 64, 1024 and 1280 (the last is past the pipelined walk), without
and with f0.  Smoothness: segments [1, 2, 37, 513, 1537] and [4609, 3] (every loop class and both sides of the k = 4 LDS-exchange
limit) on a 600 x 64 pool, max_iter = 300, without and with row_scale."""
import argparse
import os
import sys
import zlib

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from knn_svc_amd import ops

KNOB = "KNNSVC_MATCH_GENERIC_K"
DEV = "cuda"


def crc(t):
    return "%08x" % zlib.crc32(t.contiguous().cpu().numpy().tobytes())


def offsets(lens):
    seg = [0]
    for n in lens:
        seg.append(seg[-1] + n)
    return seg


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = []
    for k, generic in ((1, False), (3, False), (4, False), (4, True), (8, False)):
        tag = f"k{k}" + ("-generic" if generic else "")
        if generic:
            os.environ[KNOB] = "1"
        try:
            for dim in (64, 1024, 1280):
                if (4 * k + 2) * dim * 4 > 150 * 1024:      # the walk's LDS rule
                    continue
                gen = torch.Generator().manual_seed(100 * k + dim)
                nq, npool, seg = 130, 4000, [0, 3, 130]
                centres = torch.randn(8, dim, generator=gen)
                q = (centres[torch.randint(0, 8, (nq,), generator=gen)] + 0.7 * torch.randn(nq, dim, generator=gen)).to(DEV)
                p = (centres[torch.randint(0, 8, (npool,), generator=gen)] + 0.7 * torch.randn(npool, dim, generator=gen)).to(DEV)
                idx = torch.randint(0, npool, (nq, k), generator=gen)
                idx[::7, 0] = npool - 1                       # the clamp of "previous selection + 1"
                idx = idx.to(DEV)
                sf0 = (torch.rand(nq, generator=gen) * 200 + 100).to(DEV)
                pf0 = (torch.rand(npool, generator=gen) * 200 + 100).to(DEV)
                qn, _ = ops.row_norms(q); pn, _ = ops.row_norms(p)
                for use_f0 in (0, 1):
                    out = ops.concat_reselect_seg(idx, seg, q, qn, p, pn, sf0 if use_f0 else None, pf0 if use_f0 else None, concat_weight=0.2)
                    lines.append(f"walk   {tag:<11} dim {dim:<5} f0 {use_f0}  idx {crc(out)}")
            gen = torch.Generator().manual_seed(7 + k)
            pool = torch.rand(600, 64, generator=gen)
            pool = ((pool + torch.roll(pool, 1, 0) + torch.roll(pool, 2, 0)) / 3).to(DEV)
            for lens in ([1, 2, 37, 513, 1537], [4609, 3]):
                n = sum(lens)
                idx = torch.randint(0, 600, (n, k), generator=gen)
                idx[::50, 0] = 0; idx[::50, -1] = 599
                idx = idx.to(DEV)
                rs = (torch.rand(n, k, generator=gen) * 2 + 0.3).to(DEV)
                for scaled in (0, 1):
                    w, it = ops.smooth_weights_seg(idx, offsets(lens), pool, 0.1, max_iter=300, return_iters=True,
                                                   row_scale=rs if scaled else None)
                    lines.append(f"smooth {tag:<11} segments {str(lens):<24} row_scale {scaled}  w {crc(w)}  iterations {it.tolist()} {crc(it)}")
        finally:
            os.environ.pop(KNOB, None)
    torch.cuda.synchronize()
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
