"""Child interpreter of tests/test_gpu_pitch.py: runs every pitch-control case on the GPU and writes a JSON report
{check name: {"ok": bool, "detail": str}}; the pytest process only reads it (it must not initialise the GPU itself).

    python tests/pitch_child.py REPORT.json

The reference is tests/pitch_oracle.py fed the DEVICE's medians (the radix select has its own tests; what is judged here is the
interval and the shift).  Tolerances, none taken from what the kernel gives:
  shifted f0       largest relative error per voiced frame <= 5e-6: the bound tests/test_gpu_kernels.py uses for this stage's
                   log / exp differences (numpy's libm against the device's correctly rounded fp32 log / exp: an ulp of a log f0
                   near 6 is 4.8e-7 of the result)
  shift_semitones  within 1e-5 of the oracle's; minus the transpose (in fp32) a multiple of 12 (octave) / an integer (semitone)
Everything else is bit equality (NaN patterns included: compared as integers)."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np
import torch

import pitch_oracle as O
from knn_svc_amd import matching as M, ops
from tests.gpu_child import DEV, dev, note, run_cases, same, table, tiny_vc, write_clip

REL_TOL, SEMI_TOL = 5e-6, 1e-5
TRANSPOSES = (0.0, 3.0, -12.0, 0.5)
WORST = []


def rel_err(got, want):
    """Largest |got - want| / |want| over the voiced frames (the unvoiced ones are compared bit for bit by the caller)."""
    v = want != 0
    if got.shape != want.shape or not v.any():
        return float("inf")
    return float((np.abs(got[v].astype(np.float64) - want[v].astype(np.float64)) / np.abs(want[v].astype(np.float64))).max())


# ------------------------------------------------------------------ 1. the kernel
def case_kernel():
    cases = O.cases()
    # (a) median, t = 0 through the new entry == the old entry, bit for bit, on a stacked table with the awkward segments
    one_voiced = np.zeros(40, np.float32); one_voiced[17] = 180.0
    segs = [cases["up"][0], np.zeros(50, np.float32), cases["down"][0], one_voiced, np.array([211.0], np.float32), cases["near"][0],
            np.zeros(1, np.float32)]
    f0 = dev(np.concatenate(segs)); seg = table([len(s) for s in segs])
    pool = dev(cases["up"][1])
    qmed, pmed = ops.log_f0_median_seg(f0, seg), ops.log_f0_median(pool)
    old = ops.shift_f0_seg(f0, seg, qmed, pmed)
    new, semis = ops.shift_f0_seg(f0, seg, qmed, pmed, [0] * len(segs), [0.0] * len(segs), return_shift=True)
    new2 = ops.shift_f0_seg(f0, seg, qmed, pmed, modes=None, transposes=[0.0] * len(segs))
    q = qmed.cpu().numpy()
    note("kernel/median-t0-is-the-old-entry", same(old, new) and same(old, new2) and bool(np.isnan(q[1, 0]) and np.isnan(q[6, 0]))
         and q[3, 1] == 1 and bool(torch.isnan(old[seg[1]:seg[2]]).sum() == 0),
         f"{len(segs)} segments, {seg[-1]} rows; voiced counts {q[:, 1].tolist()}")
    # the three entries share one kernel, so the table is also held against the oracle (fed the device's medians), and every
    # segment alone through the single-sequence entry must give the stacked result
    old_h, pm, bad = old.cpu().numpy(), np.float32(pmed[0].item()), []
    for i, s in enumerate(segs):
        got = old_h[seg[i]:seg[i + 1]]
        want_i = O.shift(s, q[i, 0], pm, O.MEDIAN, 0)[0]
        unv = s == 0
        if unv.all():                                  # nothing to shift: the median is NaN and is not applied to anything
            ok = bool(np.isnan(q[i, 0]))
        else:
            WORST.append(rel_err(got, want_i))
            ok = WORST[-1] <= REL_TOL
        ok = ok and np.array_equal(got[unv].view(np.uint32), s[unv].view(np.uint32)) \
            and np.array_equal(np.isnan(got), np.isnan(want_i))          # (NaN wherever the oracle has one)
        alone = ops.shift_f0(f0[seg[i]:seg[i + 1]].contiguous(), qmed[i].contiguous(), pmed)
        if not (ok and same(alone, old[seg[i]:seg[i + 1]])):
            bad.append(i)
    note("kernel/median-t0-equals-the-oracle-and-each-segment-alone", not bad, f"segments that differ: {bad}")
    want = [(float(pmed[0]) - float(q[i, 0])) / O.S for i in range(len(segs))]
    got = semis.cpu().numpy()
    okm = all((np.isnan(w) and np.isnan(g)) or abs(w - g) <= SEMI_TOL for w, g in zip(want, got))
    note("kernel/median-t0-reports-the-interval", okm, f"device {got.tolist()} / oracle {want}")

    # (b) every mode x transpose against the oracle: per case ONE call, the source stacked 16 times with the 16 combinations
    combos = [(m, t) for m in range(4) for t in TRANSPOSES]
    for name, (src, pl, _why) in cases.items():
        f0 = dev(np.tile(src, len(combos))); seg = table([len(src)] * len(combos))
        qmed, pmed = ops.log_f0_median_seg(f0, seg), ops.log_f0_median(dev(pl))
        out, semis = ops.shift_f0_seg(f0, seg, qmed, pmed, [m for m, _ in combos], [t for _, t in combos], return_shift=True)
        out, semis = out.cpu().numpy().reshape(len(combos), -1), semis.cpu().numpy()
        qm, pm = np.float32(qmed[0, 0].item()), np.float32(pmed[0].item())
        far = O.tie_distance(qm, pm)
        note(f"kernel/{name}/precondition", min(far) >= 0.1 and same(qmed[:1].expand(len(combos), 2), qmed),
             f"device medians {qm}, {pm}: {far[0]:.3f} / {far[1]:.3f} from an octave / semitone tie")
        for k, (m, t) in enumerate(combos):
            want, wsemi = O.shift(src, qm, pm, m, t)
            e = rel_err(out[k], want)
            WORST.append(e)
            unv = src == 0
            keep = np.array_equal(out[k][unv].view(np.uint32), src[unv].view(np.uint32))
            es = abs(float(semis[k]) - float(wsemi))
            whole = float(np.float32(semis[k]) - np.float32(t))
            grid = (m != O.OCTAVE or whole % 12 == 0) and (m != O.SEMITONE or whole == round(whole)) and (m != O.NONE or whole == 0)
            note(f"kernel/{name}/mode{m}/t{t:g}", e <= REL_TOL and keep and es <= SEMI_TOL and grid,
                 f"rel {e:.2e}; unvoiced kept {keep}; semitones {float(semis[k]):.6f} / oracle {float(wsemi):.6f}")
    note("kernel/largest-oracle-error", max(WORST) <= REL_TOL, f"{max(WORST):.3e}")

    # (c) seventy segments, mixed modes and transposes, one ops call (two library calls) == each segment alone
    rng = np.random.default_rng(70)
    lens = [int(v) for v in rng.integers(1, 48, size=70)]
    lens[5], lens[64], lens[69] = 300, 513, 1                     # more than one block in either library call; a 1-frame tail
    tr = O.track(sum(lens), 150.0, 71)
    f0 = dev(tr); seg = table(lens)
    modes = [int(v) for v in rng.integers(0, 4, size=70)]
    ts = [float(v) for v in rng.choice([0.0, 0.0, 2.0, -7.0, 0.25, 36.0, -36.0], size=70)]
    pmed = ops.log_f0_median(dev(cases["near"][1]))
    qmed = ops.log_f0_median_seg(f0, seg)
    out, semis = ops.shift_f0_seg(f0, seg, qmed, pmed, modes, ts, return_shift=True)
    bad = []
    for i in range(70):
        a, b = seg[i], seg[i + 1]
        o1, s1 = ops.shift_f0_seg(f0[a:b].contiguous(), [0, b - a], qmed[i:i + 1].contiguous(), pmed, [modes[i]], [ts[i]], return_shift=True)
        if not (same(out[a:b], o1) and same(semis[i:i + 1], s1)):
            bad.append(i)
    note("kernel/seventy-segments-equal-each-alone", not bad and len(set(modes)) == 4, f"segments that differ: {bad}")

    # (d) a pool without a voiced frame: `none` never looks, `median` gives NaN on voiced frames as it always did
    src = cases["near"][0]
    f0 = dev(src); seg = [0, len(src)]
    qmed, pmed = ops.log_f0_median_seg(f0, seg), ops.log_f0_median(torch.zeros(333, device=DEV))
    none, sn = ops.shift_f0_seg(f0, seg, qmed, pmed, [3], [2.0], return_shift=True)
    med, sm = ops.shift_f0_seg(f0, seg, qmed, pmed, [0], [0.0], return_shift=True)
    v = torch.from_numpy(src != 0)
    note("kernel/unvoiced-pool", bool(torch.isnan(pmed[0])) and bool(torch.isfinite(none).all()) and float(sn) == 2.0
         and bool(torch.isnan(med.cpu()[v]).all()) and same(med.cpu()[~v], f0.cpu()[~v]) and bool(torch.isnan(sm).all())
         and same(med, ops.shift_f0_seg(f0, seg, qmed, pmed)),
         f"none: finite, {float(sn)} semitones; median: NaN on the {int(v.sum())} voiced frames")
    # refusals through ops
    refused = 0
    for kw in (dict(modes=[4]), dict(transposes=[float("nan")]), dict(transposes=[36.5]), dict(modes=[0, 1])):
        try:
            ops.shift_f0_seg(f0, seg, qmed, pmed, **kw)
        except ops.KnnSvcError:
            refused += 1
    note("kernel/ops-refuses", refused == 4, f"{refused} of 4 refused")


# ------------------------------------------------------------------ 2. product
def case_product(tmp):
    from knn_svc_amd import serving
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
    src = files[0]
    # (a) defaults, explicit defaults and no arguments: the same bits everywhere
    mk = dict(prioritize_f0=True, ckpt_type="mix", post_opt="post_opt_0.2")
    mi = lambda **kw: M.match_at_inference_time(src, pool, vc.wavlm, vc.weighting, vc.weighting, tgt_dataset_path=pool, **mk, **kw)
    of0, hw0, _a, sf0 = mi()
    of1, hw1, _a, sf1 = mi(f0_shift="median", transpose=0)
    of2, hw2, _a, sf2 = mi(f0_shift="median", transpose=0.0)
    sk = dict(ckpt_type="mix", post_opt="post_opt_0.2", save=False)
    ref = os.path.join(pool, "t0.wav")
    y0 = vc.special_match(src, ref, **sk)
    y1 = vc.special_match(src, ref, f0_shift="median", transpose=0, **sk)
    eq = [same(a[src], b[src]) for a, b in ((of0, of1), (hw0, hw1), (sf0, sf1), (of0, of2), (hw0, hw2), (sf0, sf2))] + [same(y0, y1)]
    note("product/defaults-are-bit-identical", all(eq), f"features, harmonics, shifted f0 (x2), waveform: {eq}")
    # (b) semitone against the oracle, fed the device's medians
    T = sf0[src].shape[0]
    qf0 = reqs[0][1][:T]
    vc.wavlm.set_layer_mix(M._mix_of(vc.weighting, vc.wavlm))
    f0p = M.get_complete_spk_pool(pool, vc.wavlm)[4]
    pf0 = torch.cat([f0p[k] for k in f0p], 0).contiguous()
    qm = np.float32(ops.log_f0_median(dev(qf0))[0].item()); pm = np.float32(ops.log_f0_median(pf0)[0].item())
    far = O.tie_distance(qm, pm)
    note("product/precondition", min(far) >= 0.1, f"medians {qm}, {pm}: {far[0]:.3f} / {far[1]:.3f} from an octave / semitone tie")
    e0 = rel_err(sf0[src].cpu().numpy(), O.shift(qf0, qm, pm, O.MEDIAN)[0])
    _o, _h, _a, sfs = mi(f0_shift="semitone")
    want, wsemi = O.shift(qf0, qm, pm, O.SEMITONE)
    es = rel_err(sfs[src].cpu().numpy(), want)
    ys = vc.special_match(src, ref, f0_shift="semitone", **sk)
    note("product/semitone", es <= REL_TOL and e0 <= REL_TOL and float(wsemi) == round(float(wsemi)),
         f"shifted f0 rel {es:.2e} (median: {e0:.2e}); {float(wsemi)} semitones")
    qm1 = np.float32(ops.log_f0_median(dev(qf0))[0].item())
    d = float((ys - y0).abs().max())
    note("product/semitone-changes-the-waveform", d > 0 and bool(torch.isfinite(ys).all()) and ys.shape == y0.shape and qm1 == qm,
         f"max |semitone - default| {d:.2e}")
    WORST.extend([e0, es])
    # (c) none + 12: every voiced f0 doubles
    _o, _h, _a, sfn = mi(f0_shift="none", transpose=12)
    got = sfn[src].cpu().numpy()
    v = qf0 != 0
    e2 = float(np.abs(got[v].astype(np.float64) / (2.0 * qf0[v].astype(np.float64)) - 1).max())
    note("product/none-plus-12-doubles", e2 <= REL_TOL and np.array_equal(got[~v], qf0[~v]) and int(v.sum()) > 10, f"rel {e2:.2e}")
    # (d) a batch of four requests with four settings == the four single conversions, on both routes
    tv = serving.TargetVoice(vc, pool)
    sets = [("median", 0.0), ("octave", 3.0), ("semitone", -2.0), ("none", 12.0)]
    alone = [serving.BatchConverter(vc, tv, "mix", "post_opt_0.2", f0_shift=m, transpose=t).convert([r])[0].cpu()
             for r, (m, t) in zip(reqs, sets)]
    plain = [serving.BatchConverter(vc, tv, "mix", "post_opt_0.2").convert([r])[0].cpu() for r in reqs]
    moved = [i for i in range(4) if not same(alone[i], plain[i])]
    note("product/converter/settings-change-the-output", moved == [1, 2, 3], f"sources whose waveform differs from the default: {moved}")
    for route, kw in (("lanes", dict(match="lanes")), ("segmented", dict(match="segmented", match_batch=3))):
        conv = serving.BatchConverter(vc, tv, "mix", "post_opt_0.2", **kw)
        ys4 = [y.cpu() for y in conv.convert(reqs, f0_shift=[m for m, _ in sets], transpose=[t for _, t in sets])]
        bad = [i for i in range(4) if not torch.equal(ys4[i], alone[i])]
        note(f"product/converter/{route}-batch-equals-single", not bad, f"sources that differ: {bad}")
    # (e) the queue: one batch, one request transposed, one plain
    conv = serving.BatchConverter(vc, tv, "mix", "post_opt_0.2")
    one_plain = conv.convert([reqs[2]])[0].cpu()
    one_up = conv.convert([reqs[2]], transpose=2)[0].cpu()
    rq = serving.RequestQueue(conv, max_batch=2, max_wait_ms=5000.0)       # the batch closes when it is full: nothing waits
    try:
        fa, fb = rq.submit(reqs[2], transpose=2), rq.submit(reqs[2])
        ya, yb = fa.result(timeout=60), fb.result(timeout=60)
    finally:
        rq.close()
    note("product/queue", rq.batches == [2] and torch.equal(ya, one_up) and torch.equal(yb, one_plain) and not torch.equal(ya, yb),
         f"batches {rq.batches}, max |up - plain| {float((ya - yb).abs().max()):.2e}")
    # (f) bad values are refused before a file is read
    absent = os.path.join(tmp, "absent.wav")
    n = 0
    for kw in (dict(f0_shift="fifth"), dict(transpose=float("nan")), dict(transpose=36.5)):
        for fn in (lambda: vc.special_match(absent, absent, **kw), lambda: conv.convert([absent], **kw),
                   lambda: vc.many_to_one([absent], absent, target=tv, **kw)):
            try:
                fn()
            except ValueError:
                n += 1
    note("product/refusals", n == 9, f"{n} of 9 refused with ValueError")
    note("product/largest-oracle-error", max(WORST) <= REL_TOL, f"{max(WORST):.3e}")


if __name__ == "__main__":
    sys.exit(run_cases([("kernel", case_kernel), ("product", case_product)], sys.argv[1]))
