"""CPU side of the match-rules tests (tests/test_match_rules_cpu.py, tests/match_rules_child.py): inputs, fp64 references and the
measurements that say whether an input is a fair test.  No GPU, no library call.

A. The optimiser after exactly N <= 100 iterations.  The reference's stopping rules look at iterations 1, 101, 201, ...: at
   iteration 1 the previous checkpoint is the initial 20000, so nothing can stop the loop before max_iter = N <= 100, and the
   returned weights are a smooth function of the inputs — unlike the converged endpoint, which hangs on the last bit of a flat
   loss (tests/topk_oracle.py, SMOOTH_VARIANT).  ``adam_n`` is the oracle's loop (oracle/smooth_ref.py, the same operations in the
   same order) with the best iterate's number as a second result and a switch for each mistake the bar has to catch.
B. The walk's rules.  ``walk_inputs`` builds sequences on which the thresholds of select_ref.concat_reselect are reached and
   matter (a slowly drifting query, planted jumps, neighbour lists that continue the previous frame's); ``walk_trace`` replays the
   oracle and counts its branches and margins.
C. ``median_cases`` and ``rerank_cases``: inputs whose answer is known by construction."""
from __future__ import annotations

import math

import numpy as np
import torch

from oracle import knn_ref, select_ref, smooth_ref

# ====================================================================== A. optimiser routes
SMOOTH_BAR_MAX = 4e-5          # a tenth of the project's 4e-4 convergence bar: SMOOTH_BAR may not exceed it
# One bar for every case: four times the largest device error measured on the MI355X (profiles/match_rules_errors.txt).
SMOOTH_BAR = 3.1e-5
ORACLE_BAR = 5e-6              # fp32 oracle against fp64 oracle, every case
MOVE_MIN = 0.1                 # the fp64 weights leave 1 / k by at least this much (k >= 2)

POOLS = {  # name: rows, dim, row pitch, amplitude, scale
    "feat": (600, 64, 64, 1.0, 0.1),
    "harm": (900, 49, 64, 0.02, 1000.0),      # 15 padding columns of NaN behind every row
    "wide": (300, 300, 300, 1.0, 0.1),        # past the Gram kernel's 256-column stride
}


def smooth_pool(which: str) -> torch.Tensor:
    """[rows, pitch] float32, temporally smoothed as topk_oracle.smooth_inputs does; columns dim.. of every row are NaN."""
    npool, dim, ld, amp, _ = POOLS[which]
    g = torch.Generator().manual_seed({"feat": 510, "harm": 509, "wide": 511}[which])
    pool = torch.rand(npool, dim, generator=g) * amp
    pool = (pool + torch.roll(pool, 1, 0) + torch.roll(pool, 2, 0)) / 3
    out = torch.full((npool, ld), float("nan"))
    out[:, :dim] = pool
    return out


def adam_lds_rows(k: int) -> int:
    return 144 * 1024 // (2 * k * 4)


def smooth_route(k: int, rows: int, generic: bool) -> str:
    """The loop smooth_weights_launch gives a sequence of ``rows`` rows, by its documented thresholds."""
    if rows < 2:
        return "uniform"
    if k == 4 and not generic:
        if rows <= 1536:
            return f"reg<{1 if rows <= 512 else 2 if rows <= 1024 else 3}>"
        return "adam_kernel/" + ("lds" if rows <= adam_lds_rows(4) else "global")
    return f"adam_k<{k}>/" + ("lds" if rows <= adam_lds_rows(k) else "global")


class SmoothCase:
    def __init__(self, pool, k, rows, n, generic=False, row_scale=False):
        self.pool, self.k, self.rows, self.n, self.generic, self.row_scale = pool, k, rows, n, generic, row_scale
        self.route = smooth_route(k, rows, generic)
        self.name = f"{pool}/k{k}/rows{rows}/n{n}" + ("/generic" if generic else "") + ("/row_scale" if row_scale else "")

    def inputs(self):
        """-> (idx [rows, k], pool view [npool, dim] of the padded pool, scale, row_scale or None).  Row 0 of idx holds
        0, np-1, 1, np-2, ...: its +1 neighbours meet the upper clamp.  Row 0's -1 neighbours enter no loss term (the loss reads
        shift -1 from rows 1.. only), so the last column of the last row holds 0: its -1 neighbour meets the lower clamp."""
        npool, dim, ld, amp, scale = POOLS[self.pool]
        g = torch.Generator().manual_seed(1_000_003 * SMOOTH_SEED.get(self.name, 0) + 10007 * self.k + self.rows)
        idx = torch.randint(0, npool, (self.rows, self.k), generator=g)
        edge = torch.tensor([0, npool - 1, 1, npool - 2, 2, npool - 3, 3, npool - 4])
        idx[0] = edge[:self.k]
        idx[-1, self.k - 1] = 0
        rs = torch.rand(self.rows, self.k, generator=g) * 2 + 0.3 if self.row_scale else None
        return idx, smooth_pool(self.pool)[:, :dim], scale, rs


def smooth_cases() -> list:
    out = []
    for generic, lens in ((False, [2, 3, 512, 513, 1024, 1025, 1536, 1537, 4608, 4609]), (True, [2, 1025, 4608, 4609])):
        for i, rows in enumerate(lens):
            out += [SmoothCase("feat", 4, rows, 40, generic), SmoothCase("harm", 4, rows, 40, generic),
                    SmoothCase("harm" if i % 2 else "feat", 4, rows, 10, generic)]
    for k in (1, 2, 3, 5, 6, 7, 8):
        for rows in [2, 1025] + ([adam_lds_rows(k), adam_lds_rows(k) + 1] if k in (3, 8) else []):
            out += [SmoothCase("feat", k, rows, 40), SmoothCase("harm", k, rows, 40)]
    out += [SmoothCase("harm", 4, 700, 40, row_scale=True), SmoothCase("harm", 4, 1600, 40, row_scale=True),
            SmoothCase("harm", 5, 300, 40, row_scale=True)]
    out += [SmoothCase("wide", 4, 90, 40), SmoothCase("wide", 3, 90, 40)]
    return out


# Seed variants found on the CPU by tools of this module alone (search_smooth_seeds): the first variant 0, 1, 2, ... at which the
# fp32 oracle lies within ORACLE_BAR of the fp64 one, the fp64 weights leave 1 / k by MOVE_MIN and both precisions keep the same
# best iterate.  Cases not listed use variant 0.
SMOOTH_SEED = {"harm/k4/rows513/n40": 1, "harm/k4/rows513/n10": 1}

MUTATIONS = ("no_lo_clamp", "no_hi_clamp", "drop_last_grad", "drop_first_grad", "gram_swap", "b2", "last", "rs_centre_only")


def adam_n(idx, pool, scale, n, dtype=torch.float64, row_scale=None, mutate=None):
    """oracle/smooth_ref.smooth_weights for max_iter = n <= 100 -> (softmax(best theta), number of the best iterate).
    ``mutate``: one of MUTATIONS —
      no_lo_clamp / no_hi_clamp   the neighbour index wraps round instead of stopping at the pool's first / last row
      drop_last_grad / drop_first_grad   the last / first row of theta gets no gradient
      gram_swap        in the middle pair the inner products <v0, v1> and <v0, v2> of term a's 2k vectors change places
      b2               Adam's second-moment decay 0.99 instead of 0.999
      last             the last iterate whose loss was evaluated instead of the best
      rs_centre_only   row_scale multiplies the shift-0 rows only"""
    assert n <= 100 and mutate in (None,) + MUTATIONS
    n_pool = len(pool)
    pool = pool.to(dtype)
    rs = None if row_scale is None else row_scale.to(dtype)
    gathered = {}
    for s in (-1, 0, 1):
        j = idx + s
        lo = j % n_pool if mutate == "no_lo_clamp" else torch.clamp(j, min=0)
        j = torch.where(j < 0, lo, j)
        hi = j - n_pool if mutate == "no_hi_clamp" else torch.clamp(j, max=n_pool - 1)
        j = torch.where(j > n_pool - 1, hi, j)
        gathered[s] = pool[j.reshape(-1)].reshape(idx.shape[0], idx.shape[1], pool.shape[-1])
        if rs is not None and not (mutate == "rs_centre_only" and s != 0):
            gathered[s] = gathered[s] * rs[:, :, None]
    swap = None
    if mutate == "gram_swap":
        t0 = (idx.shape[0] - 1) // 2
        v = torch.cat([gathered[-1][t0 + 1], gathered[0][t0]])            # term a's 2k vectors of pair t0
        gram = v @ v.T
        gm = gram.clone()
        gm[0, 1], gm[1, 0], gm[0, 2], gm[2, 0] = gram[0, 2], gram[0, 2], gram[0, 1], gram[0, 1]
        swap = (t0, gm - gram)
    theta = torch.zeros(idx.shape, dtype=dtype, requires_grad=True)
    opt = torch.optim.Adam([theta], lr=1e-1, betas=(0.9, 0.99 if mutate == "b2" else 0.999), eps=1e-8, weight_decay=0.0,
                           amsgrad=True)
    min_loss, best, best_it, last = 20000, theta.detach().clone(), -1, None
    for t in range(n):
        e = {s: torch.sum(gathered[s] * torch.softmax(theta, dim=1)[..., None], dim=1) for s in (-1, 0, 1)}
        term_a = scale * torch.mean((e[-1][1:] - e[0][:-1]) ** 2, dim=-1)
        term_b = scale * torch.mean((e[0][1:] - e[1][:-1]) ** 2, dim=-1)
        if swap is not None:
            w = torch.softmax(theta, dim=1)
            c = torch.cat([w[swap[0] + 1], -w[swap[0]]])
            extra = torch.zeros_like(term_a)
            extra[swap[0]] = 1.0
            term_a = term_a + extra * (scale * (c @ swap[1] @ c) / pool.shape[-1])
        loss = torch.mean(term_a) + torch.mean(term_b)
        last = theta.detach().clone()
        if loss < min_loss:
            min_loss, best, best_it = loss.item(), theta.detach().clone(), t
        opt.zero_grad()
        loss.backward()
        if mutate == "drop_last_grad":
            theta.grad[-1] = 0
        if mutate == "drop_first_grad":
            theta.grad[0] = 0
        opt.step()
    return torch.softmax(last if mutate == "last" else best, dim=1), best_it


def smooth_reference(case: SmoothCase):
    """-> (fp64 weights, iterations the loop executed, fp32 oracle's distance from them).  The oracle reports the number of the
    last iteration it began (n - 1 when it ran out of iterations); the library reports how many it executed."""
    idx, pool, scale, rs = case.inputs()
    w64, it = smooth_ref.smooth_weights(idx, pool, scale, max_iter=case.n, return_iters=True, row_scale=rs, dtype=torch.float64)
    w32 = smooth_ref.smooth_weights(idx, pool, scale, max_iter=case.n, row_scale=rs)
    assert it == case.n - 1, (case.name, it)
    return w64, it + 1, float((w32.double() - w64).abs().max())


def smooth_conditions(case: SmoothCase) -> dict:
    """What the CPU test asks of a case's inputs, measured on the oracle alone."""
    idx, pool, scale, rs = case.inputs()
    w64, b64 = adam_n(idx, pool, scale, case.n, torch.float64, rs)
    w32, b32 = adam_n(idx, pool, scale, case.n, torch.float32, rs)
    return dict(err32=float((w32.double() - w64).abs().max()), move=float((w64 - 1.0 / case.k).abs().max()), best64=b64, best32=b32)


def search_smooth_seeds(limit: int = 40) -> dict:
    """-> the SMOOTH_SEED table: per case the first variant that meets the conditions (variant 0 is left out)."""
    found = {}
    for case in smooth_cases():
        for v in range(limit):
            SMOOTH_SEED[case.name] = v
            c = smooth_conditions(case)
            if c["err32"] < ORACLE_BAR and (case.k == 1 or c["move"] >= MOVE_MIN) and c["best64"] == c["best32"]:
                break
        else:
            raise AssertionError(f"{case.name}: no variant below {limit} meets the conditions")
        if v:
            found[case.name] = v
        else:
            del SMOOTH_SEED[case.name]
    return found


# ====================================================================== C. median and re-rank
def grid_f0(j):
    """55 * 2^(j / 96) Hz in float32: an eighth of a semitone per step, so that ln and log2 of neighbouring values are 7e-3 and
    1e-2 apart — thousands of float32 steps."""
    return (55.0 * np.exp2(np.asarray(j, dtype=np.float64) / 96.0)).astype(np.float32)


def median_expected(f0: np.ndarray):
    """-> (float32(log(float64(lower median of the voiced values))) or NaN, voiced count): log is monotone, so the lower median of
    the logs is the log of the lower median."""
    v = np.sort(f0[f0 != 0])
    if len(v) == 0:
        return np.float32("nan"), 0
    return np.float32(np.log(np.float64(v[(len(v) - 1) // 2]))), len(v)


def median_cases() -> dict:
    """name -> f0 [n] float32.  ``len/N``: distinct grid values in random order, every fifth frame unvoiced from N = 1023 on."""
    rng = np.random.default_rng(96)
    out = {}
    for n in (1, 2, 1023, 1024, 1025, 2049, 5000):
        f = grid_f0(rng.permutation(n))
        if n > 2:
            f[np.arange(n) % 5 == 2] = 0.0
        out[f"len/{n}"] = f
    f = np.exp2((rng.permutation(129) - 64) / 32.0).astype(np.float32)          # 0.25 .. 4, 1.0 among them
    out["neglog/median-below-1"] = np.concatenate([f[f < 1.0], f[f >= 1.0][:20]]).astype(np.float32)
    lo, hi = f[f < 1.0], f[f > 1.0]
    out["neglog/median-is-1"] = rng.permutation(np.concatenate([lo[:40], hi[:40], [np.float32(1.0)]])).astype(np.float32)
    out["lowbyte/f0"] = (1.0 + rng.permutation(256)[:200].astype(np.float64) * 2.0 ** -23).astype(np.float32)
    # consecutive float32 values above e: their logs are 1 + (20 + 0.74 m) ulp — equal in the upper three bytes, many equal outright
    bits = np.float32(math.e).view(np.uint32) + np.uint32(30) + rng.permutation(256)[:201].astype(np.uint32)
    out["lowbyte/log"] = bits.view(np.float32)
    f = grid_f0(rng.permutation(600))
    f[rng.permutation(600)[:300]] = grid_f0(300)
    out["half-equal"] = f
    f = np.zeros(1500, dtype=np.float32)
    out["unvoiced"] = f.copy()
    f[777] = 222.5
    out["one-voiced"] = f
    return out


def rerank_inputs(k: int, nq: int):
    """-> (nn [nq, k] int64, shifted f0 [nq], pool f0 [400]).  Pool values lie on the grid above every query value; every
    seventh pool row and every fourth query frame is unvoiced; from k = 2 on every third row repeats one of its pool rows."""
    rng = np.random.default_rng(1000 * k + nq)
    pf0 = grid_f0(40 + rng.permutation(400))
    pf0[np.arange(400) % 7 == 3] = 0.0
    sf0 = grid_f0(rng.integers(0, 20, nq))
    sf0[np.arange(nq) % 4 == 1] = 0.0
    nn = rng.integers(0, 400, (nq, k))
    if k >= 2:
        nn[::3, k - 1] = nn[::3, 0]
    return nn.astype(np.int64), sf0, pf0


def rerank_expected(nn, sf0, pf0):
    """The stable argsort of |float32(log2(pf0 + 1e-5f)) - float32(log2(sf0 + 1e-5f))|, the sums and the difference in float32."""
    e = np.float32(1e-5)
    lp = np.log2((pf0 + e).astype(np.float64)).astype(np.float32)
    lq = np.log2((sf0 + e).astype(np.float64)).astype(np.float32)
    key = np.abs(lp[nn] - lq[:, None])
    assert key.dtype == np.float32
    return np.take_along_axis(nn, np.argsort(key, axis=1, kind="stable"), axis=1), key


RERANK_K = (1, 2, 31, 32, 33, 63, 64)
RERANK_NQ = (1, 3, 4, 5, 1025)


# ====================================================================== B. the walk's rules
WALK_GAP = 1e-5          # the project's margin (tests/topk_child.py): ~8 x the 1.2e-6 distance error of the device walks


def _cosd(q, p):
    """knn_ref.cosine_dist without its NaN exit (the NaN cases rank such costs instead)."""
    qn = torch.norm(q, p=2, dim=-1)
    pn = torch.norm(p, p=2, dim=-1)
    dot = -torch.cdist(q[None], p[None], p=2)[0] ** 2 + qn[:, None] ** 2 + pn[None] ** 2
    dot = dot / 2
    return 1 - dot / (qn[:, None] * pn[None])


def walk_inputs(nq: int, npool: int, dim: int, k: int, seed: int, nan_row: bool = False):
    """-> (q, pool, idx, sf0, pf0).  The pool is the 3-tap roll average of clustered features (neighbouring rows are ~0.2 apart in
    cosine distance, unrelated ones ~0.6); the query starts on a pool row and drifts by 0.16 per column and frame (baseline
    ~0.04, so that 5 x baseline falls among the costs of continuing rows) except at planted jumps to other pool rows (at 0.4 of
    the sequence, and every sixth frame from 0.6 on: the plain variant's costs below the baseline); of a frame's neighbours
    one in two frames continues a neighbour of the previous frame (its row + 1: often a repeated candidate, since the walk adds
    the same successor), one in three repeats one, the rest are random; both f0 tracks are voiced
    and slow.  Pools below 100 rows: column 0 points at the last three rows (the clamp).  ``nan_row``: one pool row is NaN and
    stands in the neighbour lists of every seventh frame."""
    from knn_svc_amd import synthetic as S
    gen = torch.Generator().manual_seed(seed)
    p = S.clustered_features(npool, dim, seed=40 + seed % 1000, n_centres=40)
    p = ((p + torch.roll(p, 1, 0) + torch.roll(p, 2, 0)) / 3).contiguous()
    jumps = ({int(nq * 0.4)} | set(range(int(nq * 0.6), nq, 6))) - {0}
    rows = torch.randint(0, npool, (nq,), generator=gen)
    steps = 0.16 * torch.randn(nq, dim, generator=gen)
    q = torch.empty(nq, dim)
    for i in range(nq):
        q[i] = p[rows[i]] + 0.3 * steps[i] if i == 0 or i in jumps else q[i - 1] + steps[i]
    idx = torch.randint(0, npool, (nq, k), generator=gen)
    u = torch.rand(nq, k, generator=gen)
    b = torch.randint(0, k, (nq, k), generator=gen)
    for i in range(1, nq):
        prev = idx[i - 1][b[i]]
        idx[i] = torch.where(u[i] < 0.5 / k, torch.clamp(prev + 1, max=npool - 1), torch.where(u[i] < 0.8 / k, prev, idx[i]))
    if npool < 100:
        idx[:, 0] = torch.randint(max(npool - 3, 0), npool, (nq,), generator=gen)
    pf0 = 180.0 * torch.exp2(0.3 * torch.sin(torch.arange(npool) / 40.0)) * (1 + 0.02 * torch.randn(npool, generator=gen))
    sf0 = 170.0 * torch.exp2(0.2 * torch.sin(torch.arange(nq) / 30.0)) * (1 + 0.01 * torch.randn(nq, generator=gen))
    if nan_row:
        r = int(torch.randint(1, npool - 1, (1,), generator=gen))
        p[r] = float("nan")
        idx[3::7, k - 1] = r
    return q, p, idx, sf0.float(), pf0.float()


def walk_trace(idx, q, pool, sf0=None, pf0=None, w: float = 0.2, weight: str = "sticky"):
    """A replay of select_ref.concat_reselect (same operations in the same order) that ranks a NaN cost as +inf with ties by
    candidate number (the rule stated above the ranking in select.hip), and counts what the oracle did.  ``weight``: "sticky"
    (the oracle), "revive" (the f0 variant's weight is 0 only on the frames whose baseline is >= 0.08) or "zero" (0 throughout).
    -> dict: sel [nq, k]; gap, the smallest difference of two consecutive sorted finite costs of distinct ids; margin, the smallest
    distance of a compared quantity from its threshold (baseline from 0.08 and cost from 5 x baseline while the weight is live,
    cost from baseline in the plain variant); repeated [nq] bool; live_low, the frames with a live weight and baseline < 0.08;
    zeroed / kept, the costs on those frames below / not below 5 x baseline; off, the frames at which a live weight was switched
    off; low_after, the frames after that with baseline < 0.08; above / below, the plain variant's costs on each side of baseline;
    nan_kept, NaN-cost candidates selected while k finite ones existed; nan_seen, frames with a NaN cost."""
    k, n_pool, use_f0 = idx.shape[1], len(pool), sf0 is not None
    if use_f0:
        lf_q = torch.log2(sf0.to(q) + 1e-5)
        lf_p = torch.log2(pf0.to(pool) + 1e-5)
    w0 = 0.0 if weight == "zero" else w
    w = w0
    sel, repeated = [idx[0]], [False]
    t = dict(gap=float("inf"), margin=float("inf"), live_low=[], zeroed=0, kept=0, off=[], low_after=[], above=0, below=0,
             nan_kept=0, nan_seen=0)
    for i in range(1, len(q)):
        cand = torch.cat([idx[i], torch.clamp(sel[-1] + 1, max=n_pool - 1)])
        cf = pool[cand]
        match = _cosd(q[i][None], cf)
        cc = _cosd(pool[sel[-1]], cf)
        base = _cosd(q[i - 1][None], q[i][None])[0, 0] * 2
        fin = cc[~torch.isnan(cc)].double()
        if use_f0:
            pitch = torch.abs(lf_p[cand][None] - lf_q[i])
            live = w > 0
            if weight == "revive":
                w = w0
            if live or weight == "revive":
                t["margin"] = min(t["margin"], abs(float(base) - 0.08))
            if base < 0.08:
                if live:
                    t["live_low"].append(i)
                    t["zeroed"] += int((fin < 5 * float(base)).sum())
                    t["kept"] += int((fin >= 5 * float(base)).sum())
                    if len(fin):
                        t["margin"] = min(t["margin"], float((fin - 5 * float(base)).abs().min()))
                elif t["off"]:
                    t["low_after"].append(i)
                cc = torch.where(cc < 5 * base, torch.zeros_like(cc), cc)
            else:
                if live:
                    t["off"].append(i)
                w = 0
            total = w * torch.median(cc, dim=0, keepdim=True).values + match + pitch
        else:
            t["above"] += int((fin > float(base)).sum())
            t["below"] += int((fin <= float(base)).sum())
            if len(fin):
                t["margin"] = min(t["margin"], float((fin - float(base)).abs().min()))
            cc = torch.where(cc > base, 1.5 * cc - base, cc)
            total = w * torch.median(cc, dim=0, keepdim=True).values + match
        cost = total[0]
        nan = torch.isnan(cost)
        cost = torch.where(nan, torch.full_like(cost, float("inf")), cost)
        order = torch.argsort(cost, stable=True)
        pick = order[:k]
        if bool(nan.any()):
            t["nan_seen"] += 1
            if int((~nan).sum()) >= k:
                t["nan_kept"] += int(nan[pick].sum())
        sel.append(cand[pick])
        repeated.append(len(set(cand.tolist())) < 2 * k)
        st, sc = cost[order].double(), cand[order]
        for a in range(2 * k - 1):
            if int(sc[a]) != int(sc[a + 1]) and math.isfinite(float(st[a + 1])):
                t["gap"] = min(t["gap"], float(st[a + 1] - st[a]))
    t["sel"], t["repeated"] = torch.stack(sel), repeated
    return t


class WalkCase:
    """One sequence, walked in both variants.  ``kernel``: "generic" (concat_reselect_kernel<k>; k = 4 reaches it under
    KNNSVC_MATCH_GENERIC_K=1) or "pipe" (the pipelined walk, k = 4, dim <= 1024)."""

    def __init__(self, kernel, k, nq, npool, dim, nan_row=False):
        self.kernel, self.k, self.nq, self.npool, self.dim, self.nan_row = kernel, k, nq, npool, dim, nan_row
        self.name = f"{kernel}/k{k}/{nq}x{npool}x{dim}" + ("/nan" if nan_row else "")

    def inputs(self):
        return walk_inputs(self.nq, self.npool, self.dim, self.k, 7000 * self.k + self.dim + self.npool + 100_000 * WALK_SEED.get(self.name, 0),
                           self.nan_row)

    @property
    def counted(self):
        """The branch counts are asked of the long sequences without NaN."""
        return self.npool >= 100 and not self.nan_row


def walk_cases() -> list:
    out = [WalkCase("generic", k, 130, 4000, 64) for k in range(1, 9)]
    out += [WalkCase("generic", 8, 130, 4000, 1024), WalkCase("generic", 5, 64, 48, 64), WalkCase("generic", 3, 130, 4000, 64, nan_row=True)]
    out += [WalkCase("pipe", 4, 130, 4000, d) for d in (36, 516, 1020, 1024)]
    out += [WalkCase("pipe", 4, 64, 48, 516), WalkCase("pipe", 4, 130, 4000, 516, nan_row=True)]
    return out


def walk_conditions(case: WalkCase, traces=None) -> list:
    """The conditions on one case's inputs (tests/test_match_rules_cpu.py, B) -> the list of those it misses (empty: a fair test)."""
    q, p, idx, sf0, pf0 = case.inputs()
    plain = walk_trace(idx, q, p) if traces is None else traces[0]
    f0 = walk_trace(idx, q, p, sf0, pf0) if traces is None else traces[1]
    miss = []
    for name, t in (("plain", plain), ("f0", f0)):
        if t["gap"] < WALK_GAP:
            miss.append(f"{name}: cost gap {t['gap']:.2e}")
        if t["margin"] < WALK_GAP:
            miss.append(f"{name}: threshold margin {t['margin']:.2e}")
    if case.nan_row:
        for name, t in (("plain", plain), ("f0", f0)):
            if t["nan_seen"] < 5 or t["nan_kept"]:
                miss.append(f"{name}: {t['nan_seen']} frames with a NaN cost, {t['nan_kept']} NaN candidates kept")
    if not case.counted:
        return miss
    if sum(plain["repeated"]) > case.nq // 2:
        miss.append(f"plain: {sum(plain['repeated'])} frames with a repeated candidate")
    if min(plain["above"], plain["below"]) < 20:
        miss.append(f"plain: {plain['above']} costs above the baseline, {plain['below']} not")
    if len(f0["live_low"]) < 20 or f0["zeroed"] < 20 or f0["kept"] < 20:
        miss.append(f"f0: {len(f0['live_low'])} live frames below 0.08, {f0['zeroed']} costs zeroed, {f0['kept']} kept")
    if len(f0["off"]) != 1 or f0["off"][0] < case.nq / 3 or len(f0["low_after"]) < 10:
        miss.append(f"f0: switched off at {f0['off']}, {len(f0['low_after'])} frames below 0.08 after it")
    revive = walk_trace(idx, q, p, sf0, pf0, weight="revive")
    if not any(f0["sel"][i].tolist() != revive["sel"][i].tolist() for i in f0["low_after"]):
        miss.append("f0: a weight that comes back selects the same rows")
    zero = walk_trace(idx, q, p, sf0, pf0, weight="zero")
    differ = sum(f0["sel"][i].tolist() != zero["sel"][i].tolist() for i in f0["live_low"])
    if differ * 10 < len(f0["live_low"]):
        miss.append(f"f0: the weight decides {differ} of {len(f0['live_low'])} live frames")
    return miss


def search_walk_seeds(limit: int = 60) -> dict:
    found = {}
    for case in walk_cases():
        for v in range(limit):
            WALK_SEED[case.name] = v
            miss = walk_conditions(case)
            if not miss:
                break
            print(case.name, v, miss, flush=True)
        else:
            raise AssertionError(f"{case.name}: no variant below {limit} meets the conditions")
        if v:
            found[case.name] = v
        else:
            del WALK_SEED[case.name]
    return found


# variants found by search_walk_seeds; cases not listed use variant 0
WALK_SEED = {"generic/k1/130x4000x64": 5, "generic/k4/130x4000x64": 1, "generic/k8/130x4000x64": 2, "generic/k8/130x4000x1024": 15,
             "pipe/k4/130x4000x516": 8, "pipe/k4/130x4000x1020": 2, "pipe/k4/130x4000x1024": 1}
