"""Child interpreter of tests/test_gpu_duration.py: runs every target_duration case on the GPU and writes a JSON report
{check name: {"ok": bool, "detail": str}}; the pytest process only reads it (it must not initialise the GPU itself).

    python tests/duration_child.py REPORT.json

The reference is tests/duration_oracle.py.  What is asked, none of it taken from what the kernel gives:
  features   BIT-IDENTICAL to the oracle rounded to fp32: both sides form the index with one correctly rounded fused
             multiply-add (the oracle exactly, in rationals), then do the same three IEEE fp64 operations in the same order
             and round once; one differing element means contraction or a different index
  f0         the voiced / unvoiced pattern exactly equal; voiced values within 1 fp32 ulp (the device's and numpy's exp / log
             each err by a few fp64 ulps, one fp32 rounding follows: adjacent floats only at a near-tie); the report records
             how many frames differ at all
Everything else (a segment alone against its slice of a stacked call, a batch against single conversions, the product chain
against the same steps by hand) is bit equality."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np
import torch

import duration_oracle as O
from knn_svc_amd import audio_io, config as C, matching as M, ops
from tests.gpu_child import dev, guarded, misaligned, note, run_cases, same, table, tiny_vc, write_clip, x_equal

F0_FRAMES = [0, 0]            # voiced frames compared / frames that differ from the oracle at all


def f0_equal(got, want):
    """(pattern equal and voiced values within 1 ulp?, detail)"""
    got = got.cpu().numpy()
    if got.shape != want.shape:
        return False, f"shape {got.shape} / {want.shape}"
    v = want > 0
    pattern = np.array_equal(got > 0, v) and np.array_equal(got[~v].view(np.uint32), want[~v].view(np.uint32))
    d = O.ulp_distance(got[v], want[v]) if pattern and v.any() else np.zeros(0, np.int64)
    F0_FRAMES[0] += int(v.sum()); F0_FRAMES[1] += int((d != 0).sum())
    worst = int(d.max()) if d.size else 0
    return pattern and worst <= 1, f"pattern {pattern}, {int(v.sum())} voiced, {int((d != 0).sum())} differ, worst {worst} ulp"


def plans(lens, scales):
    ps = [O.plan_for_scale(T, s) for T, s in zip(lens, scales)]
    return [max(1, p[0]) for p in ps], [p[1] for p in ps]


# ------------------------------------------------------------------ 1. the kernel
def case_kernel():
    rng = np.random.default_rng(2024)
    # (a) edges: one stacked call at dim 1024; every segment alone equals its slice; c = 1 returns the input
    lens = [1, 2, 2, 8, 5, 300, 300]
    scales = [2.0, 0.5, 4.0, 0.25, 1.0, 1.37, 0.73]
    outs, cs = plans(lens, scales)
    seg, oseg = table(lens), table(outs)
    xh = O.feats(seg[-1], 1024, 1)
    fh = O.track(seg[-1], 170.0, 2, run=5); fh[:5] = [210.0, 0.0, 190.0, 200.0, 0.0]       # the tiny segments see both kinds
    x, f = dev(xh), dev(fh)
    gx, gf = ops.time_scale_seg(x, f, seg, outs, cs)
    wx, wf = O.time_scale_seg(xh, fh, seg, outs, cs)
    okx, nbad = x_equal(gx, wx)
    okf, df = f0_equal(gf, wf)
    note("kernel/edges/features-bit-identical", okx and outs == [2, 1, 8, 2, 5, 411, 219], f"T' {outs}; {nbad} elements differ")
    note("kernel/edges/f0", okf, df)
    bad = []
    for i in range(len(lens)):
        ax, af = ops.time_scale(x[seg[i]:seg[i + 1]].contiguous(), f[seg[i]:seg[i + 1]].contiguous(), outs[i], cs[i])
        if not (same(ax, gx[oseg[i]:oseg[i + 1]]) and same(af, gf[oseg[i]:oseg[i + 1]])):
            bad.append(i)
    note("kernel/edges/each-segment-alone", not bad, f"segments that differ: {bad}")
    note("kernel/edges/scale-one-is-the-input", same(gx[oseg[4]:oseg[5]], x[seg[4]:seg[5]]) and same(gf[oseg[4]:oseg[5]], f[seg[4]:seg[5]]))

    # (b) dims: T = 300, s = 1.37 at 1024, the small model's width and 7 (scalar path); then with the feature pointer one float
    #     off a 16-byte boundary, which forces the unaligned path
    T = 300
    (To,), (c,) = plans([T], [1.37])
    for dim in (1024, C.WAVLM_TINY["encoder_embed_dim"], 7):
        xh = O.feats(T, dim, 10 + dim)
        want = O.features32(xh, To, c)
        gx, _ = ops.time_scale(dev(xh), None, To, c)
        okx, nbad = x_equal(gx, want)
        note(f"kernel/dims/{dim}", okx, f"{nbad} elements differ")
        xo = misaligned(xh)
        gx, _ = ops.time_scale(xo, None, To, c)
        okx, nbad = x_equal(gx, want)
        note(f"kernel/dims/{dim}-offset-pointer", okx and xo.data_ptr() % 16 == 4 and xo.is_contiguous(), f"{nbad} elements differ")

    # (c) seventy segments of 3..40 rows, mixed scales in [0.25, 4], one ops call (two library calls) == each alone
    lens = [int(v) for v in rng.integers(3, 41, size=70)]
    scales = [float(v) for v in np.exp(rng.uniform(np.log(0.25), np.log(4.0), size=70))]
    scales[0], scales[1], scales[64], scales[69] = 0.25, 4.0, 4.0, 0.25
    outs, cs = plans(lens, scales)
    seg, oseg = table(lens), table(outs)
    xh, fh = O.feats(seg[-1], 1024, 3), O.track(seg[-1], 150.0, 4, run=4)
    x, f = dev(xh), dev(fh)
    gx, gf = ops.time_scale_seg(x, f, seg, outs, cs)
    bad = []
    for i in range(70):
        ax, af = ops.time_scale(x[seg[i]:seg[i + 1]].contiguous(), f[seg[i]:seg[i + 1]].contiguous(), outs[i], cs[i])
        if not (same(ax, gx[oseg[i]:oseg[i + 1]]) and same(af, gf[oseg[i]:oseg[i + 1]])):
            bad.append(i)
    wx, wf = O.time_scale_seg(xh, fh, seg, outs, cs)
    okx, nbad = x_equal(gx, wx)
    okf, df = f0_equal(gf, wf)
    note("kernel/seventy-segments-equal-each-alone", not bad and okx and okf and min(outs) >= 1,
         f"segments that differ: {bad}; against the oracle {nbad} elements differ; f0 {df}")

    # (d) f0 edges: a melody with rests, one voiced frame, no voiced frame, a row of ties; features-NULL and f0-NULL forms
    one = np.zeros(40, np.float32); one[17] = 180.0
    tie = np.array([100.0, 0.0, 0.0, 200.0, 300.0, 0.0, 150.0, 300.0], np.float32)
    parts = [O.track(700, 180.0, 5), one, np.zeros(50, np.float32), tie]
    lens = [len(p) for p in parts]
    outs, cs = plans(lens, [1.37, 2.5, 0.73, 0.5])
    seg = table(lens)
    fh = np.concatenate(parts); xh = O.feats(seg[-1], 128, 6)
    wx, wf = O.time_scale_seg(xh, fh, seg, outs, cs)
    n0, gf = ops.time_scale_seg(None, dev(fh), seg, outs, cs)
    gx, n1 = ops.time_scale_seg(dev(xh), None, seg, outs, cs)
    bx, bf = ops.time_scale_seg(dev(xh), dev(fh), seg, outs, cs)
    okf, df = f0_equal(gf, wf)
    okx, nbad = x_equal(gx, wx)
    l1 = O.taps(len(tie), outs[3], cs[3])[3]
    note("kernel/f0-edges/features-null-form", okf and n0 is None and same(gf, bf) and bool((l1 == 0.5).all()) and int((wf > 0).sum()) > 100, df)
    note("kernel/f0-edges/f0-null-form", okx and n1 is None and same(gx, bx), f"{nbad} elements differ")

    # (e) canary: 64 guard rows of a sentinel in front of and behind both outputs stay untouched (vector and scalar path)
    for dim in (1024, 7):
        lens = [1, 2, 8, 300, 37]
        outs, cs = plans(lens, [2.0, 4.0, 0.25, 1.37, 0.73])
        seg = table(lens); N = sum(outs)
        xh, fh = O.feats(seg[-1], dim, 7), O.track(seg[-1], 200.0, 8, run=6)
        (xo, x_untouched), (fo, f_untouched) = guarded(N, dim), guarded(N)
        gx, gf = ops.time_scale_seg(dev(xh), dev(fh), seg, outs, cs, out=(xo, fo))
        wx, wf = O.time_scale_seg(xh, fh, seg, outs, cs)
        guards = x_untouched() and f_untouched()
        okx, nbad = x_equal(gx, wx)
        okf, df = f0_equal(gf, wf)
        note(f"kernel/canary/{dim}", guards and okx and okf and gx.data_ptr() == xo.data_ptr(), f"guards untouched {guards}; {nbad} differ; {df}")

    # (f) refusals through ops
    refused = 0
    x, f = dev(O.feats(10, 8, 9)), dev(O.track(10, 100.0, 9))
    for a in ((x, f, [0, 10], [0], [1.0]), (x, f, [0, 10], [5], [0.0]), (x, f, [0, 10], [5], [float("nan")]), (x, f, [0, 9], [5], [2.0]),
              (x, f[:9], [0, 10], [5], [2.0]), (x, f, [0, 10], [5, 5], [2.0]), (x.t(), None, [0, 8], [5], [2.0]), (x, f, [0, 10], [2.5], [4.0])):
        try:
            ops.time_scale_seg(*a)
        except ops.KnnSvcError:
            refused += 1
    note("kernel/ops-refuses", refused == 8, f"{refused} of 8 refused")

    # (g) the kernel's time at 1500 x 1024, s = 1.25 (HIP events, warm, median of 20): reported, not judged
    xh, fh = O.feats(1500, 1024, 11), O.track(1500, 180.0, 12)
    x, f = dev(xh), dev(fh)
    (To,), (c,) = plans([1500], [1.25])
    for _ in range(5):
        ops.time_scale(x, f, To, c)
    torch.cuda.synchronize()
    ts = []
    for _ in range(20):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); ops.time_scale(x, f, To, c); e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1) * 1e3)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(20):
        ops.time_scale(x, f, To, c)
    e1.record(); e1.synchronize()
    med = float(np.median(ts)); wrote = To * 1024 * 4
    note("kernel/timing-1500x1024-s1.25", True,
         f"median of 20: {med:.2f} us (min {min(ts):.2f}, max {max(ts):.2f}); 20 back to back: {e0.elapsed_time(e1) * 1e3 / 20:.2f} us each; "
         f"{wrote} bytes written, up to {2 * wrote} read: {wrote / med / 1e6:.3f} TB/s written at the median")
    note("kernel/f0-frames-that-differ-from-the-oracle", F0_FRAMES[1] <= F0_FRAMES[0], f"{F0_FRAMES[1]} of {F0_FRAMES[0]} voiced frames (all within 1 ulp)")


# ------------------------------------------------------------------ 2. product
def seconds_for(T, s):
    """A target_duration that upstream's arithmetic turns into round(T * s) frames for a source of T frames (half a sample
    above the frame boundary, so that int() cannot fall one sample short of it)."""
    return (round(T * s) * C.HOP + 0.5) / C.SAMPLE_RATE


def case_product(tmp):
    from knn_svc_amd import serving
    from knn_svc_amd.matcher import Tail
    from knn_svc_amd.options import Extensions
    pool = os.path.join(tmp, "tgt"); os.makedirs(pool)
    for i in range(2):
        n = 3 * 16000 + 37 * i
        write_clip(os.path.join(pool, f"t{i}.wav"), n, 900 + i, f0=O.track(n // 320 + 1, 233.0, 40 + i))
    reqs, files = [], []
    for i, n in enumerate([16000 * 2 + 11, 9000, 16000 + 641, 16000 + 2000]):
        f = O.track(n // 320 + 1, 110.0, 50 + i)
        p = os.path.join(tmp, f"s{i}.wav")
        write_clip(p, n, 700 + i, f0=f)
        files.append(p); reqs.append((M.load_utterance(p)[0], f))
    vc = tiny_vc()
    src, ref = files[0], os.path.join(pool, "t0.wav")
    mk = dict(prioritize_f0=True, ckpt_type="mix", post_opt="post_opt_0.2")
    sk = dict(ckpt_type="mix", post_opt="post_opt_0.2", save=False)
    mi = lambda **kw: M.match_at_inference_time(src, ref, vc.wavlm, vc.weighting, vc.weighting, **mk, **kw)
    tv = serving.TargetVoice(vc, pool)
    conv = serving.BatchConverter(vc, tv, "mix", "post_opt_0.2")

    # (a) defaults: without the argument, with None, with an all-None list
    of0, hw0, _a, sf0 = mi()
    of1, hw1, _a, sf1 = mi(target_duration=None)
    y0 = vc.special_match(src, ref, **sk)
    y1 = vc.special_match(src, ref, target_duration=None, **sk)
    c0 = [y.cpu() for y in conv.convert(reqs)]
    c1 = [y.cpu() for y in conv.convert(reqs, target_duration=None)]
    c2 = [y.cpu() for y in conv.convert(reqs, target_duration=[None] * 4)]
    eq = [same(of0[src], of1[src]), same(hw0[src], hw1[src]), same(sf0[src], sf1[src]), same(y0, y1)] + \
         [same(a, b) and same(a, c) for a, b, c in zip(c0, c1, c2)]
    note("product/defaults-are-bit-identical", all(eq), f"features, harmonics, shifted f0, waveform, four batch waveforms: {eq}")

    # (b) identity: the source's own length gives s = 1 and the plain conversion's bits
    T = int(sf0[src].shape[0])
    d1 = T * 320 / 16000
    yi = vc.special_match(src, ref, target_duration=d1, **sk)
    ci = conv.convert([reqs[0]], target_duration=d1)[0].cpu()
    note("product/identity", M.duration_plan(T, d1) == (T, 1.0) and same(yi, y0) and same(ci, c0[0]),
         f"T {T}, {d1!r} s; special_match {same(yi, y0)}, converter {same(ci, c0[0])}")

    # (c) chain: the product against the same steps by hand, and the stretched pair against the oracle
    vc.wavlm.set_layer_mix(M._mix_of(vc.weighting, vc.wavlm))
    qp = M.get_complete_spk_pool(src, vc.wavlm)
    qx, qf = qp[0][src], qp[4][src]
    pp = M.get_complete_spk_pool(ref, vc.wavlm)
    (pk,) = list(pp[0])
    for tag, s in (("longer", 1.25), ("shorter", 0.8)):
        d = seconds_for(T, s)
        T_out, c = M.duration_plan(T, d)
        y = vc.special_match(src, ref, target_duration=d, **sk)
        _o, _h, _a, sfd = mi(target_duration=d)
        xs, fs = ops.time_scale(qx.contiguous(), qf.contiguous(), T_out, c)
        of, hw, sf = M.match_features(xs, fs, pp[0][pk], pp[4][pk], pp[5][pk], "mix", "post_opt_0.2")
        hand = Tail(vc, False, Extensions())(of, sf, hw)
        okx, nbad = x_equal(xs, O.features32(qx.cpu().numpy(), T_out, c))
        okf, df = f0_equal(fs, O.f0(qf.cpu().numpy(), T_out, c))
        note(f"product/chain/{tag}", T_out == round(T * s) and tuple(y.shape) == (T_out * 320,) and same(y, hand) and same(sfd[src], sf)
             and sfd[src].shape[0] == T_out and okx and okf and not same(y[:1000], y0[:1000]),
             f"T {T} -> {T_out}; {y.shape[0]} samples; equals by hand {same(y, hand)}; stretched features: {nbad} differ; f0 {df}")

    # (d) a batch of four with [None, shorter, longer, None] == the four single conversions, on both routes
    Ts = [M.frames_of(len(r[0]), vc.wavlm) for r in reqs]
    durs = [None, seconds_for(Ts[1], 0.8), seconds_for(Ts[2], 1.3), None]
    want = [Ts[0], round(Ts[1] * 0.8), round(Ts[2] * 1.3), Ts[3]]
    alone = [conv.convert([r], target_duration=d)[0].cpu() for r, d in zip(reqs, durs)]
    note("product/converter/lengths", [a.shape[0] for a in alone] == [t * 320 for t in want] and same(alone[0], c0[0]) and same(alone[3], c0[3]),
         f"frames {Ts} -> {[a.shape[0] // 320 for a in alone]} (planned {want})")
    for route, kw in (("lanes", dict(match="lanes")), ("segmented", dict(match="segmented", match_batch=3))):
        cv = serving.BatchConverter(vc, tv, "mix", "post_opt_0.2", **kw)
        ys4 = [y.cpu() for y in cv.convert(reqs, target_duration=durs)]
        bad = [i for i in range(4) if not same(ys4[i], alone[i])]
        note(f"product/converter/{route}-batch-equals-single", not bad, f"sources that differ: {bad}")

    # (e) the queue: two durations and a plain request in one batch; a ratio out of bounds fails alone
    rq = serving.RequestQueue(conv, max_batch=3, max_wait_ms=5000.0)       # the batch closes when it is full: nothing waits
    try:
        futs = [rq.submit(reqs[1], target_duration=durs[1]), rq.submit(reqs[2], target_duration=durs[2]), rq.submit(reqs[3])]
        ys = [f.result(timeout=60) for f in futs]
    finally:
        rq.close()
    note("product/queue/mixed-durations-share-a-batch", rq.batches == [3] and rq.isolated == 0 and all(same(y, alone[i + 1]) for i, y in enumerate(ys)),
         f"batches {rq.batches}; samples {[y.shape[0] for y in ys]}")
    rq = serving.RequestQueue(conv, max_batch=3, max_wait_ms=5000.0)
    try:
        futs = [rq.submit(reqs[1], target_duration=durs[1]), rq.submit(reqs[2], target_duration=100.0), rq.submit(reqs[3])]
        y1, y3 = futs[0].result(timeout=60), futs[2].result(timeout=60)
        err = futs[1].exception(timeout=60)
    finally:
        rq.close()
    note("product/queue/a-bad-ratio-fails-alone", isinstance(err, ValueError) and rq.batches == [3] and rq.isolated == 0
         and same(y1, alone[1]) and same(y3, alone[3]), f"{type(err).__name__}: {err}")

    # (f) files: the written file has T_out * 320 samples under the unchanged name
    d = seconds_for(T, 1.25)
    vc.special_match(src, ref, target_duration=d, ckpt_type="mix", post_opt="post_opt_0.2", save=True)
    out = os.path.join(tmp, "s0_to_t0_knn_mix_post_opt_0.2.wav")
    n = audio_io.load_audio(out)[0].shape[-1] if os.path.isfile(out) else -1
    note("product/files", n == round(T * 1.25) * 320, f"{out}: {n} samples")

    # (g) refusals before a file is read or the encoder is used
    absent = os.path.join(tmp, "absent.wav")
    n = 0
    for kw in (dict(target_duration=0), dict(target_duration=float("nan")), dict(target_duration=True), dict(target_duration="2")):
        for fn in (lambda: vc.special_match(absent, absent, **kw), lambda: conv.convert([absent], **kw),
                   lambda: vc.many_to_one([absent], absent, target=tv, **kw)):
            try:
                fn()
            except ValueError:
                n += 1
    for fn in (lambda: vc.special_match(absent, absent, target_duration=2.0, envelope_mix=0.5),
               lambda: vc.many_to_one([absent], absent, target=tv, target_duration=2.0, envelope_mix=0.5),
               lambda: serving.BatchConverter(vc, tv, envelope_mix=0.5).convert([absent], target_duration=2.0),
               lambda: M.match_at_inference_time(absent, absent, vc.wavlm, prioritize_f0=True, src_dataset_path=tmp, target_duration=2.0)):
        try:
            fn()
        except ValueError:
            n += 1
    note("product/refusals", n == 16, f"{n} of 16 refused with ValueError")


if __name__ == "__main__":
    sys.exit(run_cases([("kernel", case_kernel), ("product", case_product)], sys.argv[1]))
