"""Child interpreter of tests/test_gpu_blend.py: runs every voice-blend case on the GPU and writes a JSON report
{check name: {"ok": bool, "detail": str}}; the pytest process only reads it (it must not initialise the GPU itself).

    python tests/blend_child.py REPORT.json

The reference is tests/blend_oracle.py.  Nothing here has a tolerance: fp64 products and sums in a fixed order, rounded once, have
one answer, so the blended features are BIT-IDENTICAL to the oracle; the blended f0 shift is bit-identical to the existing
ops.shift_f0_seg (pinned to tests/pitch_oracle.py by its own tests) called with the oracle's blended fp32 median; everything else
(a segment alone against its slice of a stacked call, a batch against single conversions, the product against the same steps by
hand, identities) is bit equality as well."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np
import torch

import blend_oracle as O
from knn_svc_amd import audio_io, config as C, matching as M, ops
from tests.gpu_child import DEV, dev, guarded, misaligned, note, run_cases, same, tiny_vc, write_clip, x_equal

NAN = float("nan")


# ------------------------------------------------------------------ 1. the kernels
def case_kernel():
    rng = np.random.default_rng(2025)
    vectors = {2: O.normalise([0.7, 0.3]), 3: O.normalise([0.2, 0.5, 0.3]), 4: O.normalise([1, 2, 3, 4])}
    # (a) dims: T = 300 at V = 2, 3, 4; dim 1024 (vector path), 49 (the harmonics' width) and 7 (scalar path); then with one
    #     voice's pointer one float off a 16-byte boundary, which forces the scalar path at dim 1024
    T = 300
    for dim in (1024, 49, 7):
        for V in (2, 3, 4):
            xh = [O.feats(T, dim, 100 * V + dim + v) for v in range(V)]
            want = O.blend(xh, vectors[V])
            okx, nbad = x_equal(ops.blend_seg([dev(x) for x in xh], [0, T], [vectors[V]]), want)
            note(f"kernel/dims/{dim}/v{V}", okx, f"{nbad} elements differ")
            xs = [dev(x) for x in xh]
            xs[V - 1] = misaligned(xh[V - 1])
            okx, nbad = x_equal(ops.blend_seg(xs, [0, T], [vectors[V]]), want)
            note(f"kernel/dims/{dim}/v{V}-offset-pointer", okx, f"{nbad} elements differ")

    # (b) edges: one call stacking segments of 1, 2, 5 and 300 rows, three voices, a different vector per segment: a one-hot
    #     vector (its segment equals its input bit for bit), a zero weight on the voice that is NaN everywhere
    lens = [1, 2, 5, 300]
    seg = O.table(lens)
    xh = [O.feats(seg[-1], 1024, 31), O.feats(seg[-1], 1024, 32), np.full((seg[-1], 1024), np.nan, np.float32)]
    xh[0][3:8, :5] = [-0.0, 1e-45, 3.0e38, -3.0e38, 1.0]          # signed zero, a subnormal, values near the fp32 maximum
    rows = [O.normalise([0.5, 0.5, 0]), (0.0, 1.0, 0.0), O.normalise([0.9, 0.1, 0.0]), O.normalise([1, 3, 0])]
    xs = [dev(x) for x in xh]
    got = ops.blend_seg(xs, seg, rows)
    okx, nbad = x_equal(got, O.blend_seg(xh, seg, rows))
    note("kernel/edges/bit-identical", okx and not bool(torch.isnan(got).any()), f"{nbad} elements differ; NaN in the output: {bool(torch.isnan(got).any())}")
    note("kernel/edges/one-hot-segment-is-its-input", same(got[seg[1]:seg[2]], xs[1][seg[1]:seg[2]]))
    bad = [i for i in range(len(lens))
           if not same(ops.blend_seg([x[seg[i]:seg[i + 1]].contiguous() for x in xs], [0, lens[i]], [rows[i]]), got[seg[i]:seg[i + 1]])]
    note("kernel/edges/each-segment-alone", not bad, f"segments that differ: {bad}")
    nan_in = ops.blend_seg(xs, seg, [O.normalise([0.5, 0.5, 1e-9])] * 4)
    note("kernel/edges/a-positive-weight-lets-nan-through", bool(torch.isnan(nan_in).all()))
    hot = ops.blend_seg([xs[2], xs[0]], seg, [(0.0, 1.0)] * 4)
    note("kernel/edges/single-term-copies-bit-for-bit", same(hot, xs[0]) and hot.data_ptr() != xs[0].data_ptr())

    # (c) seventy segments of 3..40 rows, V = 3, a vector of its own each, one ops call (two library calls) == each alone
    lens = [int(v) for v in rng.integers(3, 41, size=70)]
    seg = O.table(lens)
    rows = [O.normalise(r) for r in rng.uniform(0.0, 1.0, size=(70, 3))]
    rows[0], rows[63], rows[64], rows[69] = (1.0, 0.0, 0.0), (0.0, 0.0, 1.0), O.normalise([0, 2, 6]), (0.0, 1.0, 0.0)
    xh = [O.feats(seg[-1], 1024, 40 + v) for v in range(3)]
    xs = [dev(x) for x in xh]
    got = ops.blend_seg(xs, seg, rows)
    bad = [i for i in range(70)
           if not same(ops.blend_seg([x[seg[i]:seg[i + 1]].contiguous() for x in xs], [0, lens[i]], [rows[i]]), got[seg[i]:seg[i + 1]])]
    okx, nbad = x_equal(got, O.blend_seg(xh, seg, rows))
    note("kernel/seventy-segments-equal-each-alone", not bad and okx, f"segments that differ: {bad}; against the oracle {nbad} elements differ")

    # (d) canary: 64 guard rows of a sentinel in front of and behind the output stay untouched (vector and scalar path)
    for dim in (1024, 7):
        lens = [1, 2, 5, 300, 37]
        seg = O.table(lens); N = seg[-1]
        xh = [O.feats(N, dim, 50 + v) for v in range(4)]
        rows = [vectors[4], (0.0, 0.0, 0.0, 1.0), O.normalise([1, 0, 1, 0]), vectors[4][::-1], O.normalise([0, 1, 1, 1])]
        out, untouched = guarded(N, dim)
        got = ops.blend_seg([dev(x) for x in xh], seg, rows, out=out)
        guards = untouched()
        okx, nbad = x_equal(got, O.blend_seg(xh, seg, rows))
        note(f"kernel/canary/{dim}", guards and okx and got.data_ptr() == out.data_ptr(), f"guards untouched {guards}; {nbad} differ")

    # (e) refusals through ops (the library's own are in tests/test_blend_cpu.py)
    x = dev(O.feats(10, 8, 9))
    refused = 0
    for a in (([x, x], [0, 10], [(0.5, 0.6)]), ([x, x], [0, 10], [(1.5, -0.5)]), ([x, x], [0, 10], [(NAN, 1.0)]), ([x, x], [0, 10], [(0.0, 0.0)]),
              ([x], [0, 10], [(1.0,)]), ([x] * 5, [0, 10], [(0.2,) * 5]), ([x, x], [0, 9], [(0.5, 0.5)]), ([x, x[:9]], [0, 10], [(0.5, 0.5)]),
              ([x, x], [0, 5, 10], [(0.5, 0.5)]), ([x, x.t()], [0, 10], [(0.5, 0.5)]), ([x, x], [0, 10], [(0.5, 0.25, 0.25)])):
        try:
            ops.blend_seg(*a)
        except ops.KnnSvcError:
            refused += 1
    note("kernel/ops-refuses", refused == 11, f"{refused} of 11 refused")

    # (f) the kernel's time at 1500 x 1024, V = 2 (HIP events, warm, median of 20): reported, not judged
    xs = [dev(O.feats(1500, 1024, 60 + v)) for v in range(2)]
    out = torch.empty_like(xs[0])
    for _ in range(5):
        ops.blend_seg(xs, [0, 1500], [(0.7, 0.3)], out=out)
    torch.cuda.synchronize()
    ts = []
    for _ in range(20):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); ops.blend_seg(xs, [0, 1500], [(0.7, 0.3)], out=out); e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1) * 1e3)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(20):
        ops.blend_seg(xs, [0, 1500], [(0.7, 0.3)], out=out)
    e1.record(); e1.synchronize()
    med = float(np.median(ts)); moved = 3 * 1500 * 1024 * 4
    note("kernel/timing-1500x1024-v2", True,
         f"median of 20: {med:.2f} us (min {min(ts):.2f}, max {max(ts):.2f}); 20 back to back: {e0.elapsed_time(e1) * 1e3 / 20:.2f} us each; "
         f"{moved} bytes moved (two voices read, one output written): {moved / med / 1e6:.3f} TB/s at the median")


def case_shift():
    """ops.shift_f0_seg_blend, all four modes with transposes, three voices: per segment bit-identical to the existing
    ops.shift_f0_seg on that segment with ``pmed`` = the oracle's blended fp32 median."""
    lens = [301, 777, 257, 40, 513, 300, 1237, 64, 129, 5]
    modes = [0, 1, 2, 3, 0, 1, 2, 3, 0, 1]
    ts = [0.0, 0.0, 0.0, 0.0, 2.5, -3.0, 7.0, 1.25, -12.0, 36.0]
    rows = [O.normalise([0.7, 0.3, 0]), O.normalise([1, 1, 1]), O.normalise([0.2, 0.5, 0.3]), O.normalise([1, 2, 1]), (0.0, 1.0, 0.0),
            O.normalise([1, 0, 1]), (0.0, 0.0, 1.0), O.normalise([5, 3, 2]), O.normalise([1, 1, 0]), O.normalise([0.45, 0.1, 0.45])]
    seg = O.table(lens)
    fh = O.track(seg[-1], 123.0, 70)
    f0 = dev(fh)
    pools = [dev(O.track(n, hz, 71 + i)) for i, (n, hz) in enumerate(((2011, 233.0), (1500, 466.0), (900, 155.0)))]
    pmeds = torch.stack([ops.log_f0_median(p) for p in pools]).contiguous()
    qmed = ops.log_f0_median_seg(f0, seg)
    pm_host = [np.float32(v) for v in pmeds[:, 0].cpu().numpy()]
    got, semis = ops.shift_f0_seg_blend(f0, seg, qmed, pmeds, rows, modes, ts, return_shift=True)

    def reference(i, pm):
        pmed = torch.tensor([float(pm), 1.0], device=DEV, dtype=torch.float32)
        return ops.shift_f0_seg(f0[seg[i]:seg[i + 1]].contiguous(), [0, lens[i]], qmed[i:i + 1].contiguous(), pmed, [modes[i]], [ts[i]],
                                return_shift=True)
    bad = []
    for i in range(len(lens)):
        want, ws = reference(i, O.median(pm_host, rows[i]))
        if not (same(got[seg[i]:seg[i + 1]], want) and same(semis[i:i + 1], ws)):
            bad.append(i)
    voiced = int((fh > 0).sum())
    note("shift/equals-the-existing-shift-towards-the-blended-median", not bad and 0 < voiced < len(fh) and not bool(torch.isnan(got).any()),
         f"segments that differ: {bad}; {voiced} of {len(fh)} frames voiced; medians {[float(v) for v in pm_host]}")
    hot = [i for i, r in enumerate(rows) if sorted(r) == [0.0, 0.0, 1.0]]
    ok = all(same(got[seg[i]:seg[i + 1]], reference(i, pm_host[rows[i].index(1.0)])[0]) for i in hot)
    note("shift/one-hot-is-the-shift-towards-that-voice", ok and len(hot) == 2, f"segments {hot}")
    plain = ops.shift_f0_seg_blend(f0, seg, qmed, pmeds, rows)                       # NULL tables: all median / 0
    ok = all(same(plain[seg[i]:seg[i + 1]], ops.shift_f0_seg(f0[seg[i]:seg[i + 1]].contiguous(), [0, lens[i]], qmed[i:i + 1].contiguous(),
                                                             torch.tensor([float(O.median(pm_host, rows[i])), 1.0], device=DEV)))
             for i in range(len(lens)))
    note("shift/default-tables-are-the-median-shift", ok)
    # a NaN median: ignored under weight 0, propagated under a weight > 0 (in the three modes that read the medians)
    sick = pmeds.clone(); sick[2, 0] = NAN
    got2 = ops.shift_f0_seg_blend(f0, seg, qmed, sick, rows, modes, ts)
    zero = [i for i, r in enumerate(rows) if r[2] == 0.0]
    ok0 = all(same(got2[seg[i]:seg[i + 1]], got[seg[i]:seg[i + 1]]) for i in zero)
    okn = True
    for i in range(len(lens)):
        if rows[i][2] != 0.0:
            g, f = got2[seg[i]:seg[i + 1]], f0[seg[i]:seg[i + 1]]
            if modes[i] == 3:
                okn = okn and same(g, got[seg[i]:seg[i + 1]])
            else:
                okn = okn and bool(torch.isnan(g[f != 0]).all()) and same(g[f == 0], f[f == 0])
    note("shift/nan-median-ignored-at-weight-zero-propagates-above", ok0 and okn and zero == [0, 4, 8], f"zero-weight segments {zero}: unchanged {ok0}; others NaN {okn}")
    # seventy segments: one ops call (two library calls) == each alone
    rng = np.random.default_rng(7)
    lens70 = [int(v) for v in rng.integers(3, 41, size=70)]
    seg70 = O.table(lens70)
    rows70 = [O.normalise(r) for r in rng.uniform(0.0, 1.0, size=(70, 3))]
    m70, t70 = [int(v) for v in rng.integers(0, 4, size=70)], [float(v) for v in rng.uniform(-12, 12, size=70)]
    f70 = dev(O.track(seg70[-1], 200.0, 72, run=3))
    q70 = ops.log_f0_median_seg(f70, seg70)
    g70 = ops.shift_f0_seg_blend(f70, seg70, q70, pmeds, rows70, m70, t70)
    bad = [i for i in range(70) if not same(g70[seg70[i]:seg70[i + 1]],
                                            ops.shift_f0_seg_blend(f70[seg70[i]:seg70[i + 1]].contiguous(), [0, lens70[i]], q70[i:i + 1].contiguous(),
                                                                   pmeds, [rows70[i]], [m70[i]], [t70[i]]))]
    note("shift/seventy-segments-equal-each-alone", not bad, f"segments that differ: {bad}")


# ------------------------------------------------------------------ 2. product
def case_product(tmp):
    from knn_svc_amd import serving
    from knn_svc_amd.matcher import Tail
    from knn_svc_amd.options import Extensions
    pools = {}
    for name, hz, seed in (("A", 233.0, 900), ("B", 147.0, 910), ("C", 330.0, 920)):
        pools[name] = os.path.join(tmp, name); os.makedirs(pools[name])
        for i in range(2):
            n = 3 * 16000 + 37 * i
            write_clip(os.path.join(pools[name], f"t{i}.wav"), n, seed + i, f0=O.track(n // 320 + 1, hz, seed + 40 + i))
    reqs, files = [], []
    for i, n in enumerate([16000 * 2 + 11, 9000, 16000 + 641, 16000 + 2000]):
        f = O.track(n // 320 + 1, 110.0, 50 + i)
        p = os.path.join(tmp, f"s{i}.wav")
        write_clip(p, n, 700 + i, f0=f)
        files.append(p); reqs.append((M.load_utterance(p)[0], f))
    vc = tiny_vc()
    A, B, Cv = (serving.TargetVoice(vc, pools[k]) for k in "ABC")
    kw = dict(ckpt_type="mix", post_opt="post_opt_0.2")
    one = lambda conv, r, **k: conv.convert([r], **k)[0].cpu()
    convA, convB = serving.BatchConverter(vc, A, **kw), serving.BatchConverter(vc, B, **kw)
    yA, yB = [one(convA, r) for r in reqs], [one(convB, r) for r in reqs]

    # (a) a single TargetVoice without blend: the call as it always was (the chain by hand: encode -> match_features -> Tail)
    vc.wavlm.set_layer_mix(M._mix_of(vc.weighting, vc.wavlm))
    w0 = torch.from_numpy(reqs[0][0]).to(DEV)
    qx = vc.wavlm.encode_many([w0], max_batch=32, pow2_batches=True)[0]
    T = int(qx.shape[0])
    qf = dev(reqs[0][1][:T])
    tail = Tail(vc, False, Extensions())
    per = {k: M.match_features(qx, qf, v.feats, v.f0, v.harm, "mix", "post_opt_0.2", pool_prep=v.prep) for k, v in (("A", A), ("B", B))}
    handA = tail(*[per["A"][i] for i in (0, 2, 1)]).cpu()
    note("product/single-voice-is-unchanged", same(yA[0], handA) and same(one(convA, reqs[0], blend=None), yA[0]) and not same(yA[0], yB[0]),
         f"equals match_features -> Tail by hand {same(yA[0], handA)}")

    # (b) identities, waveform bit-identical to the single-target conversion
    AB = serving.BatchConverter(vc, [A, B], **kw)
    note("product/identity/one-zero-is-towards-A", same(one(AB, reqs[0], blend=[1, 0]), yA[0]))
    note("product/identity/zero-one-is-towards-B", same(one(AB, reqs[0], blend=[0, 1]), yB[0]))
    note("product/identity/half-half-of-A-and-A-is-A", same(one(serving.BatchConverter(vc, [A, A], **kw), reqs[0], blend=[0.5, 0.5]), yA[0]))
    y37 = one(AB, reqs[0], blend=[0.3, 0.7])
    note("product/identity/swapping-voices-and-weights", same(y37, one(serving.BatchConverter(vc, [B, A], **kw), reqs[0], blend=[0.7, 0.3]))
         and not same(y37, yA[0]) and not same(y37, yB[0]))

    # (c) [.5, .5] on (A, B) == the chain by hand, and differs from both single conversions
    half = (0.5, 0.5)
    yh = one(AB, reqs[0])                                  # the converter's default: equal weights
    of = ops.blend_seg([per["A"][0].contiguous(), per["B"][0].contiguous()], [0, T], [half])
    hw = ops.blend_seg([per["A"][1].contiguous(), per["B"][1].contiguous()], [0, T], [half])
    pmeds = torch.stack([ops.log_f0_median(A.f0), ops.log_f0_median(B.f0)]).contiguous()
    sf = ops.shift_f0_seg_blend(qf, [0, T], ops.log_f0_median_seg(qf, [0, T]), pmeds, [half])
    hand = tail(of, sf, hw).cpu()
    okx, nbad = x_equal(of, O.blend([per["A"][0].cpu().numpy(), per["B"][0].cpu().numpy()], half))
    note("product/chain-by-hand", same(yh, hand) and same(one(AB, reqs[0], blend=[0.5, 0.5]), yh) and okx and tuple(yh.shape) == (T * 320,),
         f"equals by hand {same(yh, hand)}; blended features against the oracle: {nbad} differ")
    note("product/half-half-differs-from-both", not same(yh, yA[0]) and not same(yh, yB[0])
         and not same(sf, per["A"][2]) and not same(sf, per["B"][2]))

    # (d) a batch of four sources with per-source weights on both match routes == the four single conversions (three voices)
    ABC = serving.BatchConverter(vc, [A, B, Cv], blend=[2, 1, 1], **kw)
    mixes = [[0.2, 0.5, 0.3], None, [0, 1, 0], [0.6, 0, 0.4]]
    alone = [one(ABC, r, blend=m) for r, m in zip(reqs, mixes)]
    note("product/converter/single-conversions", same(alone[2], yB[2]) and same(alone[1], one(ABC, reqs[1], blend=[0.5, 0.25, 0.25]))
         and not same(alone[0], yA[0]) and len({a.shape[0] for a in alone}) == 4)
    for route, rk in (("lanes", dict(match="lanes")), ("segmented", dict(match="segmented", match_batch=3))):
        cv = serving.BatchConverter(vc, [A, B, Cv], blend=[2, 1, 1], **kw, **rk)
        ys4 = [y.cpu() for y in cv.convert(reqs, blend=mixes)]
        bad = [i for i in range(4) if not same(ys4[i], alone[i])]
        note(f"product/converter/{route}-batch-equals-single", not bad, f"sources that differ: {bad}")

    # (e) the queue: requests with different weights (and one without) share a batch; a bad vector fails alone, at the door
    rq = serving.RequestQueue(ABC, max_batch=3, max_wait_ms=5000.0)        # the batch closes when it is full: nothing waits
    try:
        err = None
        try:
            rq.submit(reqs[0], blend=[1, 1])
        except ValueError as e:
            err = e
        futs = [rq.submit(reqs[0], blend=mixes[0]), rq.submit(reqs[1]), rq.submit(reqs[3], blend=mixes[3])]
        ys = [f.result(timeout=60) for f in futs]
    finally:
        rq.close()
    note("product/queue/mixed-weights-share-a-batch-and-a-bad-vector-fails-alone",
         isinstance(err, ValueError) and rq.batches == [3] and rq.isolated == 0 and all(same(y, alone[i]) for y, i in zip(ys, (0, 1, 3))),
         f"batches {rq.batches}; refused at the door: {err}")

    # (f) together with target_duration: the query is stretched once, in front of every voice's match
    d = (round(T * 1.25) * C.HOP + 0.5) / C.SAMPLE_RATE
    yd = one(AB, reqs[0], target_duration=d, blend=[0.3, 0.7])
    (xs,), (fs,) = M.stretch_queries([qx], [qf], [d])
    To = int(xs.shape[0])
    pd = [M.match_features(xs, fs, v.feats, v.f0, v.harm, "mix", "post_opt_0.2", pool_prep=v.prep) for v in (A, B)]
    w37 = O.normalise([0.3, 0.7])
    hand = tail(ops.blend_seg([pd[0][0].contiguous(), pd[1][0].contiguous()], [0, To], [w37]),
                ops.shift_f0_seg_blend(fs.contiguous(), [0, To], ops.log_f0_median_seg(fs.contiguous(), [0, To]), pmeds, [w37]),
                ops.blend_seg([pd[0][1].contiguous(), pd[1][1].contiguous()], [0, To], [w37])).cpu()
    note("product/with-target-duration", To == round(T * 1.25) and tuple(yd.shape) == (To * 320,) and same(yd, hand), f"T {T} -> {To}; equals by hand {same(yd, hand)}")

    # (g) files and entry points: the name carries the voices' ids, not the weights; special_match / many_to_one go the same way
    out = AB.convert_files([files[0]], blend=[0.3, 0.7])
    name = os.path.join(tmp, "s0_to_A+B_knn_mix_post_opt_0.2.wav")
    ys = vc.special_match(files[0], pools["A"], blend_with=[pools["B"]], blend=[0.3, 0.7], save=False, **kw).cpu()
    os.makedirs(os.path.join(tmp, "out"))
    m2o = vc.many_to_one(files[:2], pools["A"], os.path.join(tmp, "out"), blend_with=pools["B"], blend=[0.3, 0.7], **kw)
    y3 = vc.special_match(files[0], pools["A"], blend_with=[pools["B"], pools["C"]], ckpt_type="mix", post_opt="post_opt_0.2", save=True).cpu()
    name3 = os.path.join(tmp, "s0_to_A+B+C_knn_mix_post_opt_0.2.wav")
    note("product/files", out == [name] and os.path.isfile(name) and audio_io.load_audio(name)[0].shape[-1] == T * 320 and same(ys, y37)
         and [os.path.basename(p) for p in m2o] == ["s0_to_A+B_knn_mix_post_opt_0.2.wav", "s1_to_A+B_knn_mix_post_opt_0.2.wav"]
         and os.path.isfile(name3) and same(y3, one(serving.BatchConverter(vc, [A, B, Cv], **kw), reqs[0])),
         f"{out}; {m2o}; special_match equals the converter {same(ys, y37)}")


if __name__ == "__main__":
    sys.exit(run_cases([("kernel", case_kernel), ("shift", case_shift), ("product", case_product)], sys.argv[1]))
