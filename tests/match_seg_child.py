"""Child interpreter of tests/test_gpu_match_seg.py: runs every segmented-match-stage case on the GPU and writes a JSON report
{check name: {"ok": bool, "detail": str}}; the pytest process only reads it (it must not initialise the GPU itself).

    python tests/match_seg_child.py REPORT.json

Every comparison is exact: torch.equal on int64, the int32 view for floats (NaN medians compare too)."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch

from knn_svc_amd import matching as M, ops, synthetic as S
from tests.gpu_child import DEV, note, run_cases, same, table, tiny_vc, write_clip


def f0_track(n, gen, zero_every=5):
    f = torch.rand(n, generator=gen) * 200 + 100
    f[torch.arange(n) % zero_every == 2] = 0.0
    return f


# ------------------------------------------------------------------ 1. walk
def walk_inputs(lens, npool, dim):
    gen = torch.Generator().manual_seed(sum(lens) * 1000 + dim + npool)
    nq = sum(lens)
    p = S.clustered_features(npool, dim, seed=dim, n_centres=5)
    q = p[torch.randint(0, npool, (nq,), generator=gen)] + 0.05 * torch.randn(nq, dim, generator=gen)
    idx4 = torch.randint(0, npool, (nq, 4), generator=gen)
    idx4[:, 0] = torch.randint(max(npool - 3, 0), npool, (nq,), generator=gen)      # rows next to the pool's end: the clamp
    sf0 = torch.rand(nq, generator=gen) * 200 + 100
    sf0[torch.arange(nq) % 7 == 3] = 0.0
    pf0 = torch.rand(npool, generator=gen) * 200 + 100
    pf0[torch.arange(npool) % 6 == 1] = 0.0
    return [t.to(DEV) for t in (q, p, idx4, sf0, pf0)]


def case_walk():
    lens = [1, 2, 3, 5, 64, 257, 1]
    seg = table(lens)
    for npool in (40, 300):
        for dim in (64, 1000, 1024, 1280):
            q, p, idx4, sf0, pf0 = walk_inputs(lens, npool, dim)
            qn, _ = ops.row_norms(q); pn, _ = ops.row_norms(p)
            for use_f0 in (0, 1):
                f0a = (sf0, pf0) if use_f0 else (None, None)
                got = ops.concat_reselect_seg(idx4, seg, q, qn, p, pn, *f0a, concat_weight=0.2)
                alone = []
                for a, b in zip(seg[:-1], seg[1:]):
                    alone.append(ops.concat_reselect(idx4[a:b].contiguous(), q[a:b].contiguous(), qn[a:b].contiguous(), p, pn,
                                                     sf0[a:b].contiguous() if use_f0 else None, pf0 if use_f0 else None, concat_weight=0.2))
                bad = [i for i, (a, b) in enumerate(zip(seg[:-1], seg[1:])) if not same(got[a:b], alone[i])]
                inb = bool(((got >= 0) & (got < npool)).all())
                note(f"walk/pool{npool}/dim{dim}/f0{use_f0}", not bad and inb, f"segments that differ: {bad}; indices in range: {inb}")
                # swap segments 3 (5 rows) and 4 (64 rows): a segment's output moves with it and with nothing else
                order = [0, 1, 2, 4, 3, 5, 6]
                rows = torch.cat([torch.arange(seg[s], seg[s + 1]) for s in order]).to(DEV)
                seg2 = table([lens[s] for s in order])
                got2 = ops.concat_reselect_seg(idx4[rows].contiguous(), seg2, q[rows].contiguous(), qn[rows].contiguous(), p, pn,
                                               sf0[rows].contiguous() if use_f0 else None, pf0 if use_f0 else None, concat_weight=0.2)
                bad2 = [s for k, s in enumerate(order) if not same(got2[seg2[k]:seg2[k + 1]], alone[s])]
                note(f"walk-swapped/pool{npool}/dim{dim}/f0{use_f0}", not bad2, f"segments that differ: {bad2}")


# ------------------------------------------------------------------ 2. medians and shift
def case_median():
    lens = [1, 7, 1024, 1025, 3000]
    seg = table(lens)
    gen = torch.Generator().manual_seed(5)
    f0 = f0_track(sum(lens), gen)
    f0[seg[0]:seg[1]] = 150.0                         # one row, voiced
    f0[seg[1]:seg[2]] = 0.0                           # all unvoiced: NaN median
    f0[seg[2]:seg[3]] = 0.0; f0[seg[2] + 500] = 222.5  # a single voiced frame
    seg4 = f0[seg[4]:seg[5]]
    if int((seg4 != 0).sum()) % 2:                    # an even voiced count: the LOWER median
        seg4[int(torch.nonzero(seg4)[0])] = 0.0
    pool_f0 = f0_track(500, gen).to(DEV)
    f0 = f0.to(DEV)
    med = ops.log_f0_median_seg(f0, seg)
    pmed = ops.log_f0_median(pool_f0)
    sh = ops.shift_f0_seg(f0, seg, med, pmed)
    bad_m, bad_s = [], []
    for s, (a, b) in enumerate(zip(seg[:-1], seg[1:])):
        m1 = ops.log_f0_median(f0[a:b].contiguous())
        if not same(med[s], m1):
            bad_m.append(s)
        if not same(sh[a:b], ops.shift_f0(f0[a:b].contiguous(), m1, pmed)):
            bad_s.append(s)
    counts = med[:, 1].cpu().tolist()
    shape_ok = bool(torch.isnan(med[1, 0])) and counts[1] == 0 and counts[2] == 1 and counts[4] % 2 == 0 and counts[0] == 1
    note("median/per-segment", not bad_m, f"segments that differ: {bad_m}; voiced counts {counts}")
    note("median/cases-present", shape_ok, f"voiced counts {counts}, median of the unvoiced segment {float(med[1, 0])}")
    note("shift/per-segment", not bad_s, f"segments that differ: {bad_s}")


# ------------------------------------------------------------------ 3. smoothness weights
def smooth_pool(dim, scale_amp, seed, ld=None):
    p = S.clustered_features(400, ld or dim, seed=seed, n_centres=10) * scale_amp
    p = (p + torch.roll(p, 1, 0) + torch.roll(p, 2, 0)) / 3
    p = p.to(DEV)
    return p[:, :dim] if ld else p


def case_smooth():
    gen = torch.Generator().manual_seed(13)
    pools = {"dim64-scale0.1": (smooth_pool(64, 1.0, 3), 0.1), "dim49-ld64-scale1000": (smooth_pool(49, 0.02, 4, ld=64), 1000.0)}
    for lens in ([1, 2, 37, 512, 513, 1024, 1025, 1536, 1537], [4700, 3]):
        seg = table(lens)
        n = sum(lens)
        idx = torch.randint(0, 400, (n, 4), generator=gen)
        idx[::50] = torch.tensor([0, 399, 1, 398])                                # clamped +-1 neighbours
        idx = idx.to(DEV)
        rsc = (torch.rand(n, 4, generator=gen) * 2 + 0.3).to(DEV)
        for pname, (pool, scale) in pools.items():
            assert pool.stride(0) >= pool.shape[1]
            for rs in (None, rsc):
                w, it = ops.smooth_weights_seg(idx, seg, pool, scale, max_iter=300, return_iters=True, row_scale=rs)
                bad_w, bad_it, its = [], [], []
                for s, (a, b) in enumerate(zip(seg[:-1], seg[1:])):
                    w1, it1 = ops.smooth_weights(idx[a:b].contiguous(), pool, scale, max_iter=300, return_iters=True,
                                                 row_scale=None if rs is None else rs[a:b].contiguous())
                    its.append(int(it1))
                    if not same(w[a:b], w1):
                        bad_w.append(s)
                    if int(it[s]) != int(it1):
                        bad_it.append(s)
                tag = f"smooth/{pname}/lens{lens[0]}-{lens[-1]}/{'row_scale' if rs is not None else 'plain'}"
                note(tag + "/weights", not bad_w, f"segments that differ: {bad_w}")
                note(tag + "/iters", not bad_it, f"segments that differ: {bad_it}; single-sequence iterations {its}")
                dev1 = float((w.sum(1) - 1.0).abs().max())
                note(tag + "/rows-sum-to-1", dev1 < 1e-5, f"max |sum - 1| = {dev1:.2e}")


# ------------------------------------------------------------------ 3b. the single call in its own (smaller) workspace
def case_single_workspace():
    """knnsvc_smooth_weights is the one-segment case of the segmented call but keeps its own workspace size (no rounding of the
    segment up to 64 bytes): a workspace of exactly knnsvc_smooth_workspace_bytes(nq) bytes that starts 4 bytes behind a 64-byte
    boundary — the aligned base is then 60 bytes in, the most the size allows for — inside a buffer of sentinel bytes.  One length
    per loop variant; 4609 = ADAM_LDS_ROWS + 1, where the exchange buffer is the last region of the workspace."""
    import ctypes
    from knn_svc_amd import _lib
    lib = _lib.load()
    gen = torch.Generator().manual_seed(29)
    pool = S.clustered_features(300, 64, seed=3, n_centres=10)
    pool = ((pool + torch.roll(pool, 1, 0) + torch.roll(pool, 2, 0)) / 3).to(DEV)
    lead, trail, mark = 4, 4096, 0xA5
    for nq in (1, 2, 513, 1537, 4609):
        idx = torch.randint(0, 300, (nq, 4), generator=gen)
        idx[::50] = torch.tensor([0, 299, 1, 298])
        idx = idx.to(DEV)
        rsc = (torch.rand(nq, 4, generator=gen) * 2 + 0.3).to(DEV)
        for rs in (None, rsc):
            w_ref, it_ref = ops.smooth_weights(idx, pool, 0.1, max_iter=50, return_iters=True, row_scale=rs)
            need = lib.knnsvc_smooth_workspace_bytes(nq)
            buf = torch.full((lead + need + trail,), mark, device=DEV, dtype=torch.uint8)
            assert buf.data_ptr() % 64 == 0
            w = torch.empty(nq, 4, device=DEV, dtype=torch.float32)
            it = torch.zeros(1, device=DEV, dtype=torch.int32)
            rc = lib.knnsvc_smooth_weights(ops._p(idx), nq, ops._p(pool), 300, 64, pool.stride(0), 0.1, ops._p(rs), 50, ops._p(w), ops._p(it),
                                           ctypes.c_void_p(buf.data_ptr() + lead), need, ops._stream())
            torch.cuda.synchronize()
            clean = bool((buf[:lead] == mark).all()) and bool((buf[lead + need:] == mark).all())
            ok = rc == 0 and same(w, w_ref) and int(it) == int(it_ref) and clean
            note(f"single_ws/nq{nq}/{'row_scale' if rs is not None else 'plain'}", ok,
                 f"rc {rc}, workspace {need} bytes, weights equal {same(w, w_ref)}, iterations {int(it)} / {int(it_ref)}, sentinels intact {clean}")


# ------------------------------------------------------------------ 4. wrapper chunking
def case_chunking():
    lens = [1 + i % 3 for i in range(70)]
    seg = table(lens)
    q, p, idx4, sf0, pf0 = walk_inputs(lens, 300, 64)
    qn, _ = ops.row_norms(q); pn, _ = ops.row_norms(p)
    got = ops.concat_reselect_seg(idx4, seg, q, qn, p, pn, sf0, pf0, concat_weight=0.2)
    pool = smooth_pool(64, 1.0, 3)
    w, it = ops.smooth_weights_seg(idx4, seg, pool, 0.1, max_iter=300, return_iters=True)
    med = ops.log_f0_median_seg(sf0, seg)
    sh = ops.shift_f0_seg(sf0, seg, med, med[0])
    bad = {"walk": [], "w": [], "it": [], "med": [], "shift": []}
    for s, (a, b) in enumerate(zip(seg[:-1], seg[1:])):
        r = ops.concat_reselect(idx4[a:b].contiguous(), q[a:b].contiguous(), qn[a:b].contiguous(), p, pn, sf0[a:b].contiguous(), pf0,
                                concat_weight=0.2)
        w1, it1 = ops.smooth_weights(idx4[a:b].contiguous(), pool, 0.1, max_iter=300, return_iters=True)
        m1 = ops.log_f0_median(sf0[a:b].contiguous())
        for key, ok in (("walk", same(got[a:b], r)), ("w", same(w[a:b], w1)), ("it", int(it[s]) == int(it1)), ("med", same(med[s], m1)),
                        ("shift", same(sh[a:b], ops.shift_f0(sf0[a:b].contiguous(), m1, med[0].contiguous())))):
            if not ok:
                bad[key].append(s)
    note("chunking/70-segments", not any(bad.values()), f"segments that differ: {bad}")


# ------------------------------------------------------------------ 5. match_features_many
def case_match_many():
    lens = [1, 2, 31, 150, 151, 600]
    gen = torch.Generator().manual_seed(77)
    P = S.clustered_features(2000, 256, seed=21, n_centres=20).to(DEV)
    P2 = S.clustered_features(2000, 256, seed=22, n_centres=20).to(DEV)
    Pf0 = f0_track(2000, gen, zero_every=9).to(DEV)
    Ph = (torch.rand(2000, 49, generator=gen) * 0.02).to(DEV)
    qs, f0s = [], []
    for i, n in enumerate(lens):
        rows = torch.randint(0, 2000, (n,), generator=gen)
        qs.append((P.cpu()[rows] + 0.05 * torch.randn(n, 256, generator=gen)).to(DEV))
        f0s.append(f0_track(n, gen, zero_every=4 + i).to(DEV))
    prep = M.prepare_pool(P)
    nn_all, _fl = M.batched_knn(torch.cat(qs, 0).contiguous(), P, prep)
    nn = [t.contiguous() for t in nn_all.split(lens)]
    runs = [(ck, po, None) for ck in ("mix", "wavlm_only") for po in ("post_opt_0.2", "no_post_opt")] + [("mix", "post_opt_0.2", P2)]
    for ck, po, synth in runs:
        kw = dict(pool_prep=prep, return_debug=True)
        if synth is not None:
            kw["synth_list"] = synth
        many = M.match_features_many(qs, f0s, P, Pf0, Ph, ck, po, nn32s=nn, **kw)
        bad = []
        for i in range(len(lens)):
            one = M.match_features(qs[i], f0s[i], P, Pf0, Ph, ck, po, nn32=nn[i], **kw)
            for k, name in enumerate(("out_feats", "harm", "shifted_f0")):
                if not same(many[i][k], one[k]):
                    bad.append((i, name))
            for key in one[3]:
                a, b = many[i][3][key], one[3][key]
                ok = same(a, b) if isinstance(b, torch.Tensor) or b is None else (a == b)
                if not ok:
                    bad.append((i, key))
        note(f"match_many/{ck}/{po}/{'synth' if synth is not None else 'same-pool'}", not bad, f"(item, tensor) that differ: {bad}")
    # without neighbour lists: one search over the stacked frames, same neighbours as the search above
    many = M.match_features_many(qs, f0s, P, Pf0, Ph, "mix", "post_opt_0.2", pool_prep=prep, return_debug=True)
    note("match_many/own-search", all(same(many[i][3]["nn32"], nn[i]) for i in range(len(lens))), "")


# ------------------------------------------------------------------ 6. product
def case_product(tmp):
    from knn_svc_amd import serving
    pool = os.path.join(tmp, "tgt"); os.makedirs(pool)
    for i in range(4):
        write_clip(os.path.join(pool, f"t{i}.wav"), 3 * 16000 + 37 * i, 900 + i)
    srcd = os.path.join(tmp, "src"); os.makedirs(srcd)
    lens = [16000 * 2 + 11, 16000 * 3, 9000, 16000 * 2 + 11, 16000 + 641, 40000]
    files = []
    for i, n in enumerate(lens):
        files.append(os.path.join(srcd, f"s{i}.wav"))
        write_clip(files[-1], n, 700 + i, f0_mul=1.2)
    for ckpt_type, kind in (("mix", "mix"), ("wavlm_only", "f0")):
        vc = tiny_vc(kind)
        tv = serving.TargetVoice(vc, pool)
        lanes = [y.cpu() for y in serving.BatchConverter(vc, tv, ckpt_type, "post_opt_0.2", match="lanes").convert(files)]
        conv = serving.BatchConverter(vc, tv, ckpt_type, "post_opt_0.2", match="segmented", match_batch=4)
        assert conv.match == "segmented" and conv.match_batch == 4
        for rep in range(3):
            seg = [y.cpu() for y in conv.convert(files)]
            bad = [i for i in range(len(files)) if not same(seg[i], lanes[i])]
            note(f"product/{ckpt_type}/convert/run{rep}", not bad and len(seg) == len(files), f"sources that differ: {bad}")
        a = vc.many_to_one(files, pool, os.path.join(tmp, f"out_lanes_{kind}"), ckpt_type=ckpt_type, match="lanes", target=tv)
        os.environ["KNNSVC_MATCH"] = "segmented"; os.environ["KNNSVC_MATCH_BATCH"] = "4"
        try:
            b = vc.many_to_one(files, pool, os.path.join(tmp, f"out_seg_{kind}"), ckpt_type=ckpt_type, target=tv)
        finally:
            del os.environ["KNNSVC_MATCH"], os.environ["KNNSVC_MATCH_BATCH"]
        bad = [os.path.basename(x) for x, y in zip(a, b) if open(x, "rb").read() != open(y, "rb").read()]
        note(f"product/{ckpt_type}/many_to_one-files", not bad and len(a) == len(b) == len(files), f"files that differ: {bad}")


if __name__ == "__main__":
    cases = [("walk", case_walk), ("median", case_median), ("smooth", case_smooth), ("single_ws", case_single_workspace), ("chunking", case_chunking),
             ("match_many", case_match_many), ("product", case_product)]
    sys.exit(run_cases(cases, sys.argv[1]))
