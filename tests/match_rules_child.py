"""Child interpreter of tests/test_gpu_match_rules.py: the match stage's rules and optimiser routes against fp64 / the CPU oracle.

    python tests/match_rules_child.py REPORT.json

smooth/   every loop route of smooth_weights_launch after exactly N iterations (N = 40, and 10 on the k = 4 routes) against
          oracle/smooth_ref.smooth_weights(..., dtype=float64): max|w - w64| < SMOOTH_BAR, N iterations executed, rows sum to 1
          within 1e-6, max_iter = -N gives the same bits, max_iter = 1 gives exactly 1 / k.  The route is the one the documented
          thresholds give (k, rows, KNNSVC_MATCH_GENERIC_K); the library has no call that names it.
walk/     concat_reselect_kernel<k> for k = 1..8 and the pipelined walk at dims 36 / 516 / 1020 / 1024 on sequences that reach the
          thresholds (tests/match_rules_oracle.py, B): sets equal to select_ref.concat_reselect on every frame, rows equal in order
          wherever the candidates are distinct (long pools), indices in range; with a NaN pool row, equal to the replay that ranks
          NaN costs as +inf, and the NaN row never kept.
median/   log_f0_median: within one float32 step of float32(log(float64(lower median))), the voiced count exact.
rerank/   f0_rerank for k up to 64: exactly the stable argsort of the float32 keys.

What makes an input a fair test (oracle stability, branch counts, margins) is asserted on the CPU (tests/test_match_rules_cpu.py);
the margins are asserted again here, next to the comparison they license.  The first exception ends the run."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np
import torch

import match_rules_oracle as R
from knn_svc_amd import ops
from oracle import select_ref
from tests.gpu_child import DEV, note, run_cases

KNOB = "KNNSVC_MATCH_GENERIC_K"


class generic_k:
    """KNNSVC_MATCH_GENERIC_K=1 inside the block when ``on`` (the library reads it per call)."""

    def __init__(self, on=True):
        self.on = on

    def __enter__(self):
        if self.on:
            os.environ[KNOB] = "1"

    def __exit__(self, *a):
        os.environ.pop(KNOB, None)


# ------------------------------------------------------------------ A. optimiser routes
def case_smooth():
    pools = {name: R.smooth_pool(name).to(DEV) for name in R.POOLS}
    print(f"{'case':44s} {'route':20s} {'device':>9s} {'fp32 oracle':>11s} {'bar':>8s}")
    for case in R.smooth_cases():
        idx, _, scale, rs = case.inputs()
        w64, it_ref, e32 = R.smooth_reference(case)
        pool = pools[case.pool][:, :R.POOLS[case.pool][1]]
        idx_d, rs_d = idx.to(DEV), None if rs is None else rs.to(DEV)
        with generic_k(case.generic):
            assert R.smooth_route(case.k, case.rows, os.environ.get(KNOB) == "1") == case.route
            w, it = ops.smooth_weights(idx_d, pool, scale, max_iter=case.n, return_iters=True, row_scale=rs_d)
            forced = ops.smooth_weights(idx_d, pool, scale, max_iter=-case.n, row_scale=rs_d)
            first = ops.smooth_weights(idx_d, pool, scale, max_iter=1, row_scale=rs_d)
        e = float((w.cpu().double() - w64).abs().max())
        rows1 = float((w.double().sum(1) - 1.0).abs().max())
        same_forced = torch.equal(w.view(torch.int32), forced.view(torch.int32))
        uniform = bool((first.cpu() == torch.tensor(np.float32(1.0) / np.float32(case.k))).all())
        print(f"{case.name:44s} {case.route:20s} {e:9.2e} {e32:11.2e} {R.SMOOTH_BAR:8.1e}")
        ok = e < R.SMOOTH_BAR and int(it) == it_ref and rows1 < 1e-6 and same_forced and uniform and tuple(w.shape) == tuple(idx.shape)
        note(f"smooth/{case.name}", ok, f"route {case.route}: max|w - w64| {e:.2e} (fp32 oracle {e32:.2e}, bar {R.SMOOTH_BAR:.1e}), "
                                        f"iterations {int(it)} / {it_ref}, max|row sum - 1| {rows1:.1e}, max_iter = -N same bits "
                                        f"{same_forced}, max_iter = 1 gives 1/k {uniform}")


# ------------------------------------------------------------------ B. the walk's rules
def case_walk():
    for case in R.walk_cases():
        q, p, idx, sf0, pf0 = case.inputs()
        qd, pd = q.to(DEV), p.to(DEV)
        qn, _ = ops.row_norms(qd); pn, _ = ops.row_norms(pd)
        nan_rows = torch.isnan(p).any(1).nonzero().flatten().tolist()
        for use_f0 in (0, 1):
            f0c = (sf0, pf0) if use_f0 else (None, None)
            tag = f"walk/{case.name}/f0{use_f0}"
            t = R.walk_trace(idx, q, p, *f0c)
            ref = t["sel"]
            if not case.nan_row:
                assert torch.equal(ref, select_ref.concat_reselect(idx.clone(), q, p, *f0c, concat_weight=0.2)), tag + ": the replay is not the oracle"
            assert t["gap"] >= R.WALK_GAP and t["margin"] >= R.WALK_GAP, f"{tag}: oracle gap {t['gap']:.2e}, threshold margin {t['margin']:.2e}"
            with generic_k(case.kernel == "generic" and case.k == 4):
                assert case.kernel == "generic" or (case.k == 4 and case.dim <= 1024 and KNOB not in os.environ)
                got = ops.concat_reselect(idx.to(DEV), qd, qn, pd, pn, *(x.to(DEV) if x is not None else None for x in f0c),
                                          concat_weight=0.2).cpu()
            inb = bool(((got >= 0) & (got < case.npool)).all()) and tuple(got.shape) == (case.nq, case.k)
            sets = [i for i in range(case.nq) if sorted(got[i].tolist()) != sorted(ref[i].tolist())]
            ordered = case.npool >= 100
            rows = [i for i in range(case.nq) if ordered and not t["repeated"][i] and got[i].tolist() != ref[i].tolist()]
            nan_kept = int(sum((got == r).sum() for r in nan_rows)) if t["nan_kept"] == 0 else 0
            exact = sum(not r for r in t["repeated"]) if ordered else 0
            note(tag, inb and not sets and not rows and not nan_kept,
                 f"frames whose set differs {sets[:8]}, whose order differs {rows[:8]} ({exact} of {case.nq} frames compared in order), in "
                 f"range {inb}, NaN rows kept {nan_kept} ({t['nan_seen']} frames with a NaN cost); oracle gap {t['gap']:.2e}, threshold "
                 f"margin {t['margin']:.2e}")


# ------------------------------------------------------------------ C. median and re-rank
def case_median():
    for name, f0 in R.median_cases().items():
        want, count = R.median_expected(f0)
        res = ops.log_f0_median(torch.from_numpy(f0).to(DEV)).cpu().numpy()
        if count == 0:
            ok, d = bool(np.isnan(res[0])), 0.0
        else:
            d = abs(float(res[0]) - float(want))
            ok = d <= float(np.spacing(np.abs(want)))
        note(f"median/{name}", ok and float(res[1]) == count, f"median {res[0]!r} / expected {want!r} (|d| {d:.1e}), voiced {res[1]:.0f} / {count}")


def case_rerank():
    for k in R.RERANK_K:
        for nq in R.RERANK_NQ:
            nn, sf0, pf0 = R.rerank_inputs(k, nq)
            want, _ = R.rerank_expected(nn, sf0, pf0)
            got = ops.f0_rerank(torch.from_numpy(nn).to(DEV), torch.from_numpy(sf0).to(DEV), torch.from_numpy(pf0).to(DEV)).cpu().numpy()
            bad = int((got != want).any(axis=1).sum()) if got.shape == want.shape else -1
            note(f"rerank/k{k}/nq{nq}", bad == 0, f"rows that differ from the stable argsort: {bad} of {nq}")


if __name__ == "__main__":
    sys.exit(run_cases([("median", case_median), ("rerank", case_rerank), ("walk", case_walk), ("smooth", case_smooth)], sys.argv[1],
                       autograd=("smooth",)))          # the fp64 reference differentiates its loss
