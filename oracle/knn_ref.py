"""Oracle: cosine-distance kNN (reference lib_ongaku_test.py:148-175 and the
driver loop ddsp_prematch_dataset.py:1195-1210).  Test infrastructure only."""
from __future__ import annotations

import numpy as np
import torch


def cosine_dist(q: torch.Tensor, p: torch.Tensor) -> torch.Tensor:
    """One call of fast_cosine_dist on <= 20 query rows:
        d = 1 - ((-cdist(q,p)^2 + |q|^2 + |p|^2) / 2) / (|q| |p|)
    torch.cdist picks its mm route when either side has > 25 rows
    (sqrt(clamp_min([-2q, |q|^2, 1] @ [p, 1, |p|^2]^T, 1e-30))) and the direct
    sqrt(sum((x-y)^2)) route otherwise — both are reached on the path (pool
    vs 8 candidates).  NaN => the reference exits; here it raises."""
    qn = torch.norm(q, p=2, dim=-1)
    pn = torch.norm(p, p=2, dim=-1)
    dot = -torch.cdist(q[None], p[None], p=2)[0] ** 2 + qn[:, None] ** 2 + pn[None] ** 2
    dot = dot / 2
    d = 1 - dot / (qn[:, None] * pn[None])
    if torch.isnan(d).any():
        raise FloatingPointError("containing nan")
    return d


def cosine_dist_all(q: torch.Tensor, p: torch.Tensor, rows: int = 20) -> torch.Tensor:
    """fast_cosine_dist's internal 20-row stepping (lib_ongaku_test.py:154-175)."""
    return torch.cat([cosine_dist(q[s:s + rows], p) for s in range(0, len(q), rows)], 0)


def knn_topk(q: torch.Tensor, pool: torch.Tensor, k: int = 32, rows: int = 20):
    """Ascending-distance top-k per query row, computed 20 rows at a time
    (ddsp_prematch_dataset.py:1195-1210).  Returns (idx int64 [Nq,k], dist f32 [Nq,k])."""
    idx, val = [], []
    for s in range(0, len(q), rows):
        t = cosine_dist(q[s:s + rows], pool).topk(k=k, dim=-1, largest=False)
        idx.append(t.indices)
        val.append(t.values)
    return torch.cat(idx, 0), torch.cat(val, 0)


def cosine_dist_f64(q: torch.Tensor, p: torch.Tensor) -> np.ndarray:
    """Mathematically exact (fp64) cosine distance; used to measure whether an index
    mismatch sits inside an fp32 rounding gap (SURVEY.md §7 hard part 1)."""
    qd = q.double().numpy()
    pd = p.double().numpy()
    qn = np.linalg.norm(qd, axis=1)
    pn = np.linalg.norm(pd, axis=1)
    return 1.0 - (qd @ pd.T) / (qn[:, None] * pn[None])


def topk_agreement(idx_a: torch.Tensor, idx_b: torch.Tensor, dist_f64: np.ndarray, tau: float = 5e-7):
    """Parity statistics between two [Nq,k] index sets.

    Returns dict with: exact row-match rate for the first 4 and all k columns
    (ordered), set-match rate, and ``max_gap`` = the largest fp64 distance
    inversion any mismatch implies (a mismatch is *explained* when the two
    candidates' exact distances differ by <= tau, i.e. they sit inside one
    fp32 rounding gap of the reference formula)."""
    a = idx_a.numpy().astype(np.int64)
    b = idx_b.numpy().astype(np.int64)
    nq, k = a.shape
    top4 = float(np.mean(np.all(a[:, :4] == b[:, :4], axis=1)))
    allk = float(np.mean(np.all(a == b, axis=1)))
    sets = float(np.mean([set(a[i]) == set(b[i]) for i in range(nq)]))
    da = np.take_along_axis(dist_f64, a, axis=1)
    db = np.take_along_axis(dist_f64, b, axis=1)
    # position-wise exact-distance difference: identical rankings give 0
    max_gap = float(np.max(np.abs(da - db)))
    unexplained = int(np.sum(np.abs(da - db) > tau))
    return dict(top4=top4, allk=allk, sets=sets, max_gap=max_gap, unexplained=unexplained)


# ---------------------------------------------------------------- exact oracle of the search (knnsvc_knn_rescore's claim)
def _sortable(d: np.ndarray) -> np.ndarray:
    """Order-preserving uint32 image of fp32 distances (knn.hip: sortable)."""
    u = np.ascontiguousarray(d, dtype=np.float32).view(np.uint32)
    return np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def _ulp(x: np.ndarray) -> np.ndarray:
    return np.spacing(np.abs(x).astype(np.float32)).astype(np.float64)


def ref_distance_f32(dot, qsq, psq, qn, pn) -> np.ndarray:
    """knn.hip ref_distance in IEEE fp32, every operation rounded on its own and in the kernel's order (contraction off):
        r = (-2 dot + |q|^2) + |p|^2 ; cd = sqrt(max(r, 1e-30)) ; dp = ((-(cd cd) + qn qn) + pn pn) / 2 ; d = 1 - dp / (qn pn)
    dot [rows, cols]; qsq / qn [rows, 1]; psq / pn [1, cols] — all float32."""
    f = np.float32
    dot = dot.astype(f)
    r = (f(-2.0) * dot + qsq) + psq
    cd = np.sqrt(np.maximum(r, f(1e-30)))
    dp = ((-(cd * cd)) + qn * qn) + pn * pn
    dp = dp / f(2.0)
    return (f(1.0) - dp / (qn * pn)).astype(f)


def exact_distance_matrix(q, p, qn, qsq, pn, psq, mask=None, rows: int = 64) -> np.ndarray:
    """[nq, np] fp32 distances the search claims to rank by: q.p in fp64 (torch, on the tensors' own device, query rows in chunks
    of ``rows``), rounded ONCE to fp32, then ref_distance_f32 with the given fp32 norms (take them from ops.row_norms on the same
    tensors, so that only the search is under test).  ``mask`` = (lo, hi): those pool rows sit at exactly 1."""
    nq, npool = q.shape[0], p.shape[0]
    f = np.float32
    qn_ = qn.detach().cpu().numpy().astype(f)[:, None]
    qs_ = qsq.detach().cpu().numpy().astype(f)[:, None]
    pn_ = pn.detach().cpu().numpy().astype(f)[None, :]
    ps_ = psq.detach().cpu().numpy().astype(f)[None, :]
    pd = p.detach().double()
    out = np.empty((nq, npool), dtype=f)
    for r0 in range(0, nq, rows):
        r1 = min(nq, r0 + rows)
        dot = (q[r0:r1].detach().double() @ pd.T).float().cpu().numpy()         # fp64 sums, one rounding to fp32
        out[r0:r1] = ref_distance_f32(dot, qs_[r0:r1], ps_, qn_[r0:r1], pn_)
    del pd
    if mask is not None and mask[0] < mask[1]:
        out[:, max(0, mask[0]):max(0, min(npool, mask[1]))] = f(1.0)
    return out


def exact_topk_from(D: np.ndarray, k: int):
    """Top-k of every row of an exact distance matrix by (distance bits, lower index) -> (idx int64 [nq, k], dist f32 [nq, k])."""
    nq, npool = D.shape
    keys = (_sortable(D).astype(np.uint64) << np.uint64(32)) | np.arange(npool, dtype=np.uint64)[None, :]
    part = np.partition(keys, k - 1, axis=1)[:, :k] if k < npool else keys
    part = np.sort(part, axis=1)
    idx = (part & np.uint64(0xFFFFFFFF)).astype(np.int64)
    return idx, np.take_along_axis(D, idx, axis=1)


def exact_rescore_topk(q, p, qn, qsq, pn, psq, k, mask=None):
    """The exact top-k the kNN search must return: ``exact_distance_matrix`` + ``exact_topk_from``."""
    return exact_topk_from(exact_distance_matrix(q, p, qn, qsq, pn, psq, mask), k)


def compare_to_exact(idx, dist, D: np.ndarray, k: int, idx_offset: int = 0) -> dict:
    """A search's lists (idx [nq, k] with ``idx_offset`` added, dist [nq, k]) against the exact oracle ``D``.
      rows_equal   rows whose indices AND distance bits equal the oracle's
      mismatches   (row, position) entries that differ from the oracle in index or distance bits
      unexplained  mismatches NOT explained by a double-rounding tie: explained only where the oracle distances of the two indices
                   involved — and the returned distance — lie within 1 fp32 ulp of each other.  Expect 0.
      left_out     pool rows outside a returned list whose oracle distance is below that row's k-th returned distance.  Expect 0.
      bad_lists    rows with an index out of range or listed twice."""
    ia = np.asarray(idx.cpu() if hasattr(idx, "cpu") else idx).astype(np.int64) - idx_offset
    da = np.asarray(dist.cpu() if hasattr(dist, "cpu") else dist).astype(np.float32)
    nq, npool = D.shape
    oi, od = exact_topk_from(D, k)
    bad = int(np.sum((ia.min(1) < 0) | (ia.max(1) >= npool) | np.array([len(set(r)) != k for r in ia])))
    ia_c = np.clip(ia, 0, npool - 1)
    same = (ia == oi) & (da.view(np.uint32) == od.view(np.uint32))
    a = np.take_along_axis(D, ia_c, axis=1).astype(np.float64)          # oracle distance of the returned index
    b = od.astype(np.float64)                                           # oracle distance at that position
    tol = np.maximum(_ulp(a), _ulp(b))
    explained = (np.abs(a - b) <= tol) & (np.abs(da.astype(np.float64) - a) <= tol)
    mism = ~same
    outside = D.copy()
    np.put_along_axis(outside, ia_c, np.float32(np.inf), axis=1)
    left_out = int(np.sum(outside < da[:, k - 1:k]))
    return dict(rows_equal=int(np.sum(same.all(1))), rows=nq, mismatches=int(mism.sum()),
                unexplained=int(np.sum(mism & ~explained)), left_out=left_out, bad_lists=bad)
