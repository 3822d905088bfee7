"""The inputs of tests/match_rules_child.py are fair tests — asserted on the CPU oracle alone (tests/match_rules_oracle.py), no GPU.

A. every optimiser case: the fp32 oracle within 5e-6 of the fp64 one, the fp64 weights at least 0.1 from uniform, the same best
   iterate in both precisions, a best iterate that is not the last in some N = 10 case, every loop route present — and the bar
   catches each of eight mistakes by a factor of ten.
B. every walk case: the oracle's cost gaps and threshold margins >= 1e-5, at least 20 live frames below 0.08 with 20 costs zeroed
   and 20 kept, one switch-off past a third of the sequence with 10 low frames behind it, a weight that decides 10 % of the live
   frames, 20 plain costs on each side of the baseline.
C. the median and re-rank inputs hold the edge cases their names promise."""
import numpy as np
import pytest
import torch

import match_rules_oracle as R
from oracle import select_ref, smooth_ref


# ------------------------------------------------------------------ A
@pytest.fixture(scope="module")
def smooth_conditions():
    return {c.name: R.smooth_conditions(c) for c in R.smooth_cases()}


def test_smooth_bar_is_within_the_allowed_maximum():
    assert 0 < R.SMOOTH_BAR <= R.SMOOTH_BAR_MAX == 4e-5


def test_smooth_cases_cover_every_route():
    cases = R.smooth_cases()
    assert len({c.name for c in cases}) == len(cases)
    by_route = {}
    for c in cases:
        by_route.setdefault(c.route, set()).add((c.rows, c.n, c.row_scale))
    k4 = {"reg<1>": (2, 3, 512), "reg<2>": (513, 1024), "reg<3>": (1025, 1536), "adam_kernel/lds": (1537, 4608), "adam_kernel/global": (4609,),
          "adam_k<4>/lds": (2, 1025, 4608), "adam_k<4>/global": (4609,)}
    for route, lens in k4.items():
        for rows in lens:
            assert {(rows, 40, False), (rows, 10, False)} <= by_route[route], (route, rows)
    for k in (1, 2, 3, 5, 6, 7, 8):
        assert {(2, 40, False), (1025, 40, False)} <= by_route[f"adam_k<{k}>/lds"]
    for k in (3, 8):
        assert (18432 // k, 40, False) in by_route[f"adam_k<{k}>/lds"] and (18432 // k + 1, 40, False) in by_route[f"adam_k<{k}>/global"]
    scaled = {c.route.split("<")[0].split("/")[0] for c in cases if c.row_scale}
    assert scaled == {"reg", "adam_kernel", "adam_k"}
    assert {c.pool for c in cases} == {"feat", "harm", "wide"}


def test_smooth_inputs_reach_both_clamps_and_pad_with_nan():
    for c in R.smooth_cases():
        idx, pool, scale, rs = c.inputs()
        npool, dim, ld, _, _ = R.POOLS[c.pool]
        assert idx[0].tolist() == [0, npool - 1, 1, npool - 2, 2, npool - 3, 3, npool - 4][:c.k] and int(idx[-1, -1]) == 0
        assert tuple(pool.shape) == (npool, dim) and pool.stride(0) == ld and bool(torch.isfinite(pool).all())
    assert bool(torch.isnan(R.smooth_pool("harm")[:, 49:]).all()) and R.smooth_pool("harm").shape[1] == 64


def test_smooth_oracle_is_stable_and_moves(smooth_conditions):
    bad = {n: c for n, c in smooth_conditions.items()
           if not (c["err32"] < R.ORACLE_BAR and c["best64"] == c["best32"] and (n.split("/")[1] == "k1" or c["move"] >= R.MOVE_MIN))}
    assert not bad, bad


def test_smooth_best_iterate_is_not_always_the_last(smooth_conditions):
    early = [n for n, c in smooth_conditions.items() if n.split("/")[3] == "n10" and c["best64"] < 9]
    assert early, "no N = 10 case whose best iterate is not the last"


def test_adam_n_is_the_oracle_loop_and_dtype_defaults_to_float32():
    c = R.SmoothCase("harm", 5, 300, 40, row_scale=True)
    idx, pool, scale, rs = c.inputs()
    for dtype in (torch.float32, torch.float64):
        w, it = smooth_ref.smooth_weights(idx, pool, scale, max_iter=40, return_iters=True, row_scale=rs, dtype=dtype)
        assert w.dtype == dtype and it == 39 and torch.equal(w, R.adam_n(idx, pool, scale, 40, dtype, rs)[0])
    assert torch.equal(smooth_ref.smooth_weights(idx, pool, scale, max_iter=40, row_scale=rs),
                       smooth_ref.smooth_weights(idx, pool, scale, max_iter=40, row_scale=rs, dtype=torch.float32))


MUTATION_CASES = [R.SmoothCase("feat", 4, 3, 40), R.SmoothCase("harm", 4, 513, 40), R.SmoothCase("feat", 4, 1536, 10),
                  R.SmoothCase("feat", 2, 2, 40), R.SmoothCase("harm", 5, 300, 40, row_scale=True)]


def test_the_bar_catches_each_mutation_tenfold():
    assert {c.name for c in MUTATION_CASES} <= {c.name for c in R.smooth_cases()}
    moved = {m: 0.0 for m in R.MUTATIONS}
    for c in MUTATION_CASES:
        idx, pool, scale, rs = c.inputs()
        w64, _ = R.adam_n(idx, pool, scale, c.n, torch.float64, rs)
        for m in R.MUTATIONS:
            if (m == "rs_centre_only" and rs is None) or (m == "gram_swap" and c.k < 2):
                continue
            wm, _ = R.adam_n(idx, pool, scale, c.n, torch.float64, rs, mutate=m)
            moved[m] = max(moved[m], float((wm - w64).abs().max()))
    print({m: f"{v:.2e}" for m, v in moved.items()})
    assert all(v >= 10 * R.SMOOTH_BAR for v in moved.values()), moved


# ------------------------------------------------------------------ B
def test_walk_cases_cover_the_shapes():
    cases = R.walk_cases()
    long = {(c.kernel, c.k, c.dim) for c in cases if c.counted}
    assert {("generic", k, 64) for k in range(1, 9)} | {("generic", 8, 1024)} | {("pipe", 4, d) for d in (36, 516, 1020, 1024)} <= long
    assert all((c.nq, c.npool) == (130, 4000) for c in cases if c.counted)
    for kernel in ("generic", "pipe"):
        assert any(c.kernel == kernel and c.npool == 48 for c in cases) and any(c.kernel == kernel and c.nan_row for c in cases)
    # the pipelined walk's column split: an odd number of float4 granules, and both sides of 256 columns per half
    halves = {d: ((d // 4 + 1) // 2) * 4 for d in (36, 516, 1020, 1024)}
    assert [(d // 4) % 2 for d in (36, 516, 1020)] == [1, 1, 1] and halves[36] < 256 < halves[516] and halves[1020] == halves[1024] == 512


@pytest.mark.parametrize("case", R.walk_cases(), ids=lambda c: c.name)
def test_walk_inputs_reach_the_rules_with_margin(case):
    q, p, idx, sf0, pf0 = case.inputs()
    traces = (R.walk_trace(idx, q, p), R.walk_trace(idx, q, p, sf0, pf0))
    if not case.nan_row:
        assert torch.equal(traces[0]["sel"], select_ref.concat_reselect(idx.clone(), q, p, concat_weight=0.2))
        assert torch.equal(traces[1]["sel"], select_ref.concat_reselect(idx.clone(), q, p, sf0, pf0, concat_weight=0.2))
    else:
        r = torch.isnan(p).any(1).nonzero().flatten()
        assert len(r) == 1 and not any(bool((t["sel"] == r).any()) for t in traces)
    if case.npool < 100:
        assert bool((idx[:, 0] >= case.npool - 3).all()) and any(traces[0]["repeated"])
    miss = R.walk_conditions(case, traces)
    assert not miss, miss


# ------------------------------------------------------------------ C
def test_median_cases_hold_their_edges():
    cases = R.median_cases()
    assert [len(cases[f"len/{n}"]) for n in (1, 2, 1023, 1024, 1025, 2049, 5000)] == [1, 2, 1023, 1024, 1025, 2049, 5000]
    counts = {n: R.median_expected(f)[1] for n, f in cases.items()}
    assert {c % 2 for c in counts.values() if c > 2} == {0, 1} and counts["unvoiced"] == 0 and counts["one-voiced"] == 1
    assert np.isnan(R.median_expected(cases["unvoiced"])[0])
    neg = cases["neglog/median-below-1"]
    assert 0.25 <= neg.min() and neg.max() <= 4 and R.median_expected(neg)[0] < 0
    assert R.median_expected(cases["neglog/median-is-1"])[0] == 0 and (cases["neglog/median-is-1"] < 1).any()
    low = cases["lowbyte/f0"].view(np.uint32)
    assert len(set(low >> 8)) == 1 and len(set(low)) == len(low)
    logs = np.log(cases["lowbyte/log"].astype(np.float64)).astype(np.float32).view(np.uint32)
    assert len(set(logs >> 8)) == 1 and 50 < len(set(logs)) < len(logs)
    half = cases["half-equal"]
    assert (half == R.grid_f0(300)).sum() >= 300 and R.median_expected(half)[0] == np.float32(np.log(np.float64(R.grid_f0(300))))
    for n, f in cases.items():          # on the grid the neighbours of the median are thousands of float32 steps away
        if n.startswith("len/") and counts[n] > 2:
            v = np.sort(f[f != 0]); m = (len(v) - 1) // 2
            assert np.log(np.float64(v[m + 1])) - np.log(np.float64(v[m])) > 1000 * np.spacing(np.float32(np.log(np.float64(v[m]))))


def test_rerank_cases_hold_their_edges():
    for k in R.RERANK_K:
        for nq in R.RERANK_NQ:
            nn, sf0, pf0 = R.rerank_inputs(k, nq)
            want, key = R.rerank_expected(nn, sf0, pf0)
            assert nn.shape == (nq, k) and sorted(want[0].tolist()) == sorted(nn[0].tolist())
            gaps = np.diff(np.sort(key, axis=1), axis=1)
            assert not ((gaps > 0) & (gaps < 5e-3)).any()            # distinct keys are a grid step (1 / 96) apart, or equal
            voiced_q = sf0 != 0
            assert (pf0[pf0 != 0].min() > sf0.max())                 # the pool lies on one side of every query value
            if nq >= 3:
                assert (~voiced_q).any() and voiced_q.any()
            if k >= 31:
                assert (gaps == 0).any() and (pf0[nn] == 0).any()
            if k >= 2:
                assert nn[0, 0] == nn[0, k - 1]
    assert (np.array(R.RERANK_NQ) % 4 != 0).sum() >= 3
