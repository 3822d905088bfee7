"""Child interpreter of tests/test_gpu_harmony.py: runs every harmony case on the GPU and writes a JSON report
{check name: {"ok": bool, "detail": str}}; the pytest process only reads it (it must not initialise the GPU itself).

    python tests/harmony_child.py REPORT.json

The reference is tests/harmony_oracle.py fed the DEVICE's lead f0 (shift and correction have their own tests; what is judged here
is the part).  Tolerances, none taken from what the kernel gives:
  notes t, D       exactly equal (D = the part's notes minus the notes knnsvc_tune_f0_seg reports for the same mask and tuning):
                   tests/test_harmony_cpu.py shows that every kernel case stands >= 1e-6 semitone from every note decision going
                   the other way, the product cases check the same here on the device's f0 before they compare, and an ulp of the
                   device's fp64 log moves a pitch by 1e-13; behind the note everything is integer arithmetic
  unpitched frames bit-equal to the input
  pitched f0       largest relative error <= 5e-6, tests/tune_child.py's bound and for its reason: the device's fp64 log / exp
                   against numpy's (the glide is a contraction, so a difference does not grow; what remains is the final fp32
                   rounding)
  identities       chromatic: within the same 5e-6 of (float)exp(l + steps * S); steps = +-d: of twice / half the lead
  mix_waves        bit-equal to numpy fp64: products and sums only, one rounding
Everything else is bit equality."""
import ctypes
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np
import torch

import harmony_oracle as HO
import pitch_oracle as P
import tune_oracle as O
from knn_svc_amd import config as C, matching as M, ops
from knn_svc_amd.options import Harmony, HarmonyPart, HarmonyShift, Tuning
from tests.gpu_child import DEV, dev, guarded, misaligned, note, run_cases, same, table, tiny_vc, write_clip, x_equal

REL_TOL = 5e-6
MARGIN_MIN = 1e-6
WORST = []


def shift(p):
    """The oracle's part as the options.HarmonyShift the code under test takes."""
    return None if p is None else HarmonyShift(p.mask, p.steps, p.alpha, p.log_ref)


def lead_tuning(p):
    """A hard-snap Tuning of the part's scale and tuning frequency: its notes are the lead's n."""
    return None if p is None or p.steps == 0 else Tuning(p.scale, 1.0, 0.0, p.tuning_hz)


def against_oracle(f0_host, seg, parts, got, got_notes, lead=None):
    """-> (ok, detail): t exactly (and D exactly, against the device's lead notes, where given), unpitched frames bit for bit,
    pitched f0 within REL_TOL; the oracle's margin is part of the verdict."""
    want, wt, wD, on, margin = HO.harmony(f0_host, seg, parts)
    got, gt = got.cpu().numpy(), got_notes.cpu().numpy()
    if got.shape != want.shape or gt.shape != wt.shape or gt.dtype != np.int32:
        return False, f"shapes {got.shape} {gt.shape} {gt.dtype}"
    notes_bad = int((gt != wt).sum())
    D_bad = 0 if lead is None else int(((gt - lead.cpu().numpy())[on] != wD[on]).sum())
    keep = np.array_equal(got[~on].view(np.uint32), np.asarray(f0_host, np.float32)[~on].view(np.uint32))
    e = float((np.abs(got[on].astype(np.float64) - want[on].astype(np.float64)) / want[on].astype(np.float64)).max()) if on.any() else 0.0
    WORST.append(e)
    return (notes_bad == 0 and D_bad == 0 and keep and e <= REL_TOL and margin >= MARGIN_MIN,
            f"{int(on.sum())} moved frames; notes that differ {notes_bad}; D that differ {D_bad}; others kept {keep}; rel {e:.2e}; margin {margin:.2e}")


# ------------------------------------------------------------------ 1. the kernel
def case_kernel():
    from knn_svc_amd import _lib
    cases = HO.kernel_cases()
    # (a) edges: one stacked table, input one float off a 16-byte boundary
    f0h, seg, parts, why = HO.edges()
    sh = [shift(p) for p in parts]
    f0 = misaligned(f0h)
    got, notes = ops.harmony_f0_seg(f0, seg, sh, return_notes=True)
    _y, lead = ops.tune_f0_seg(f0, seg, [lead_tuning(p) for p in parts], return_notes=True)
    ok, detail = against_oracle(f0h, seg, parts, got, notes, lead)
    note("kernel/edges/equals-the-oracle", ok, detail)
    # the library call itself, writing into guarded rows of f0 and of notes
    lib = _lib.load()
    n = len(seg) - 1
    out, untouched = guarded(f0h.size)
    nbuf = torch.full((f0h.size + 128,), -77, device=DEV, dtype=torch.int32)
    ws_bytes = lib.knnsvc_tune_f0_workspace_bytes(f0h.size, n)
    ws = torch.full((ws_bytes + 512,), 0x5A, device=DEV, dtype=torch.uint8)
    live = [p if p is not None else HarmonyShift(0, 0, 1.0, 0.0) for p in sh]
    rc = lib.knnsvc_harmony_f0_seg(f0.data_ptr(), (ctypes.c_int64 * (n + 1))(*seg), n, (ctypes.c_int32 * n)(*[p.mask for p in live]),
                                   (ctypes.c_int32 * n)(*[p.steps for p in live]), (ctypes.c_double * n)(*[p.alpha for p in live]),
                                   (ctypes.c_double * n)(*[p.log_ref for p in live]), out.data_ptr(), nbuf[64:].data_ptr(), ws[256:].data_ptr(),
                                   ws_bytes, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    note("kernel/edges/guards-untouched", rc == 0 and untouched() and same(out, got) and same(nbuf[64:64 + f0h.size], notes)
         and bool((nbuf[:64] == -77).all()) and bool((nbuf[64 + f0h.size:] == -77).all())
         and bool((ws[:256] == 0x5A).all()) and bool((ws[256 + ws_bytes:] == 0x5A).all()),
         f"rc {rc}; workspace {ws_bytes} bytes for {f0h.size} frames")
    offs = [s for s, p in enumerate(parts) if p is None or p.steps == 0]
    note("kernel/edges/off-segments-keep-their-bits", len(offs) == 2 and all(same(got[seg[s]:seg[s + 1]], f0[seg[s]:seg[s + 1]])
                                                                              and bool((notes[seg[s]:seg[s + 1]] == -1).all()) for s in offs),
         "; ".join(why[s] for s in offs))
    bad = []
    for s in range(n):
        a, b = seg[s], seg[s + 1]
        if s in offs:
            continue
        y1, n1 = ops.harmony_f0_seg(f0[a:b].contiguous(), [0, b - a], [sh[s]], return_notes=True)
        if not (same(y1, got[a:b]) and same(n1, notes[a:b])):
            bad.append(s)
    note("kernel/edges/each-segment-alone-is-bit-identical", not bad, f"segments that differ: {bad}")
    again, notes2 = ops.harmony_f0_seg(f0, seg, sh, return_notes=True)
    note("kernel/edges/second-call-is-bit-identical", same(again, got) and same(notes2, notes) and same(ops.harmony_f0_seg(f0, seg, sh), got))

    # (b) the stepwise melody under every mask, step and glide (96 segments: two library calls), the long run, the low melody
    for name in ("steps", "one-run", "low"):
        f0h, seg, parts = cases[name]
        f0 = dev(f0h)
        got, notes = ops.harmony_f0_seg(f0, seg, [shift(p) for p in parts], return_notes=True)
        _y, lead = ops.tune_f0_seg(f0, seg, [lead_tuning(p) for p in parts], return_notes=True)
        ok, detail = against_oracle(f0h, seg, parts, got, notes, lead)
        note(f"kernel/{name}/equals-the-oracle", ok, f"{len(parts)} settings x {seg[1]} frames; " + detail)
        # the identities, judged without the oracle: chromatic = a parallel part; steps = +-d = an octave
        g, x = got.cpu().numpy().astype(np.float64), f0h.astype(np.float64)
        nt, ld = notes.cpu().numpy(), lead.cpu().numpy()
        worst_par = worst_oct = 0.0
        cnt_par = cnt_oct = bad_D = 0
        for s, p in enumerate(parts):
            a, b = seg[s], seg[s + 1]
            on = f0h[a:b] > 0
            d = len(HO.degrees(p.mask))
            if d == 12:
                want = HO.parallel(f0h[a:b], p.steps).astype(np.float64)
                worst_par = max(worst_par, float((np.abs(g[a:b][on] - want[on]) / want[on]).max()))
                bad_D += int(((nt[a:b] - ld[a:b])[on] != p.steps).sum())
                cnt_par += int(on.sum())
            if abs(p.steps) == d:
                ratio = 2.0 if p.steps > 0 else 0.5
                worst_oct = max(worst_oct, float(np.abs(g[a:b][on] / x[a:b][on] / ratio - 1.0).max()))
                bad_D += int(((nt[a:b] - ld[a:b])[on] != (12 if p.steps > 0 else -12)).sum())
                cnt_oct += int(on.sum())
        note(f"kernel/{name}/chromatic-is-a-parallel-part", cnt_par > 0 and worst_par <= REL_TOL and bad_D == 0,
             f"{cnt_par} frames, rel {worst_par:.2e}; D off {bad_D}")
        note(f"kernel/{name}/d-steps-are-an-octave", cnt_oct > 0 and worst_oct <= REL_TOL and bad_D == 0, f"{cnt_oct} frames, rel {worst_oct:.2e}")
    note("kernel/largest-oracle-error", max(WORST) <= REL_TOL, f"{max(WORST):.3e}")

    # (c) seventy segments, mixed on / off / scales, one ops call (two library calls) == each segment alone
    rng = np.random.default_rng(70)
    lens = [int(v) for v in rng.integers(1, 48, size=70)]
    lens[5], lens[64], lens[69] = 300, 1100, 1                    # more than 1024 frames in a segment of the second call; a 1-frame tail
    f0 = dev(P.track(sum(lens), 150.0, 71)); seg = table(lens)
    pick = [None, HarmonyShift(0xFFF, 0, 1.0, 0.0)] + [shift(HO.P(*a)) for a in (("chromatic", 4), ("C:major", 2, 0.0), ("G:major", -5, 189.8),
                                                                                   (O.CUSTOM, 7, 40.0, 432.0))]
    sh = [pick[int(v)] for v in rng.integers(0, len(pick), size=70)]
    sh[64], sh[69] = pick[4], pick[2]
    got, notes = ops.harmony_f0_seg(f0, seg, sh, return_notes=True)
    bad = []
    for i in range(70):
        a, b = seg[i], seg[i + 1]
        y1, n1 = ops.harmony_f0_seg(f0[a:b].contiguous(), [0, b - a], [sh[i]], return_notes=True)
        if n1 is None:                                     # off alone: the input itself, no notes
            okk = y1.data_ptr() == f0[a:b].data_ptr() and same(got[a:b], f0[a:b]) and bool((notes[a:b] == -1).all())
        else:
            okk = same(got[a:b], y1) and same(notes[a:b], n1)
        if not okk:
            bad.append(i)
    kinds = len({id(p) for p in sh})
    note("kernel/seventy-segments-equal-each-alone", not bad and kinds == len(pick), f"segments that differ: {bad}; {kinds} kinds of setting")
    half = [None] * 64 + sh[64:]
    g2, n2 = ops.harmony_f0_seg(f0, seg, half, return_notes=True)
    note("kernel/all-off-chunk-is-copied", same(g2[:seg[64]], f0[:seg[64]]) and bool((n2[:seg[64]] == -1).all())
         and same(g2[seg[64]:], got[seg[64]:]) and same(n2[seg[64]:], notes[seg[64]:]))
    y0 = ops.harmony_f0_seg(f0, seg, [None, pick[1]] * 35)
    y1, n1 = ops.harmony_f0_seg(f0, seg, [None] * 70, return_notes=True)
    note("kernel/all-off-returns-the-input-object", y0 is f0 and y1 is f0 and n1 is None)

    # (d) refusals through ops
    refused = 0
    p = pick[2]
    for args in ((f0, seg, [p] * 69), (f0.to(torch.int32), seg, [p] * 70), (f0[:100].contiguous(), seg, [p] * 70)):
        try:
            ops.harmony_f0_seg(*args)
        except ops.KnnSvcError:
            refused += 1
    note("kernel/ops-refuses", refused == 3, f"{refused} of 3 refused")


# ------------------------------------------------------------------ 2. the mix
def case_mix():
    rng = np.random.default_rng(5)
    gains4 = [1.0, 10.0 ** (-6.0 / 20.0), 10.0 ** (-9.0 / 20.0), 0.3]
    for n in (1, 3, 1023, 64001):
        ys = [rng.standard_normal(n).astype(np.float32) for _ in range(4)]
        d = [dev(y) for y in ys]
        ok4, bad4 = x_equal(ops.mix_waves(d, gains4), HO.mix(ys, gains4))
        ok1, bad1 = x_equal(ops.mix_waves(d[:1], [0.7]), HO.mix(ys[:1], [0.7]))
        # misaligned voices and output: one float off a 16-byte boundary each, and a mix of aligned and misaligned
        m = [misaligned(y) for y in ys]
        out = misaligned(np.zeros(n, np.float32))
        okm, badm = x_equal(ops.mix_waves(m[:3], gains4[:3], out=out), HO.mix(ys[:3], gains4[:3]))
        okx, badx = x_equal(ops.mix_waves([d[0], m[1]], gains4[:2]), HO.mix(ys[:2], gains4[:2]))
        # a voice with gain 0 is not read: it holds NaN
        nan = torch.full((n,), float("nan"), device=DEV)
        okz, badz = x_equal(ops.mix_waves([d[0], nan, d[2]], [0.5, 0.0, 0.25]), HO.mix([ys[0], None, ys[2]], [0.5, 0.0, 0.25]))
        # in place: the output is the first voice, then the last
        first, last = d[0].clone(), d[2].clone()
        r1 = ops.mix_waves([first, d[1], d[2]], gains4[:3], out=first)
        r2 = ops.mix_waves([d[0], d[1], last], gains4[:3], out=last)
        want = HO.mix(ys[:3], gains4[:3])
        oki = r1 is first and r2 is last and x_equal(first, want)[0] and x_equal(last, want)[0]
        out_g, untouched = guarded(n)
        ops.mix_waves(d, gains4, out=out_g)
        note(f"mix/{n}-samples", ok4 and ok1 and okm and okx and okz and oki and untouched() and x_equal(out_g, HO.mix(ys, gains4))[0],
             f"samples that differ: 4 voices {bad4}, 1 voice {bad1}, misaligned {badm} / {badx}, zero-gain NaN voice {badz}; in place {oki}")
    refused = 0
    y = dev(np.zeros(8, np.float32))
    for ys, g in (([y, y], [1.0]), ([y, y], [1.0, -1.0]), ([y, y], [0.0, 0.0]), ([y, y[:4]], [1.0, 1.0]), ([y], [float("nan")])):
        try:
            ops.mix_waves(ys, g)
        except ops.KnnSvcError:
            refused += 1
    note("mix/ops-refuses", refused == 5, f"{refused} of 5 refused")


# ------------------------------------------------------------------ 3. product
def case_product(tmp):
    from knn_svc_amd import serving
    from tune_child import sharp_track
    pools = {}
    for name, hz, seed in (("A", 233.0, 900), ("B", 147.0, 910)):
        pools[name] = os.path.join(tmp, name); os.makedirs(pools[name])
        for i in range(2):
            n = 3 * 16000 + 37 * i
            write_clip(os.path.join(pools[name], f"t{i}.wav"), n, seed + i, f0=P.track(n // 320 + 1, hz, seed + 40 + i))
    reqs, files = [], []
    for i, n in enumerate([16000 * 2 + 11, 9000, 16000 + 641]):
        f = sharp_track(n // 320 + 1, 50 + i)
        p = os.path.join(tmp, f"s{i}.wav")
        write_clip(p, n, 700 + i, f0=f)
        files.append(p); reqs.append((M.load_utterance(p)[0], f))
    vc = tiny_vc()
    kw = dict(ckpt_type="mix", post_opt="post_opt_0.2")
    vc.wavlm.set_layer_mix(M._mix_of(vc.weighting, vc.wavlm))
    A, B = (serving.TargetVoice(vc, pools[k]) for k in "AB")
    H1 = Harmony((2,), scale="C:major")
    H3 = Harmony((HarmonyPart(2, -6.0), HarmonyPart(-3, -9.0), HarmonyPart(-7, -12.0)), scale="A:minor", lead_db=-1.0, glide_ms=0.0)
    conv = serving.BatchConverter(vc, A, **kw)

    # (a) defaults, explicit None and "off": the same bits
    y_plain = [conv.convert([r])[0] for r in reqs]
    ref = os.path.join(pools["A"], "t0.wav")
    sk = dict(save=False, **kw)
    eq = [same(y_plain[0], conv.convert([reqs[0]], harmony=None)[0]), same(y_plain[0], conv.convert([reqs[0]], harmony="off")[0]),
          same(y_plain[0], serving.BatchConverter(vc, A, harmony=None, **kw).convert([reqs[0]])[0]),
          same(y_plain[0], serving.BatchConverter(vc, A, harmony=H1, **kw).convert([reqs[0]], harmony="off")[0]),
          same(vc.special_match(files[0], ref, **sk), vc.special_match(files[0], ref, harmony=None, **sk))]
    note("product/defaults-are-bit-identical", all(eq), f"convert None / off, converter None / off, special_match None: {eq}")

    # (b) stems: the lead is the conversion without harmony; the mix is numpy's fp64 mix of the stems
    def mix_check(key, cv, plain, h):
        st = cv.convert([reqs[0]], harmony=h, stems=True)[0]
        out = cv.convert([reqs[0]], harmony=h)[0]
        want = dev(HO.mix([s.cpu().numpy() for s in st[1:]], h.gains))
        if cv.ext.loudness_db is not None:
            ops.normalize_loudness(want, cv.ext.loudness_db, vc.sr, out=want)
        if cv.ext.peak_db is not None:
            want = ops.limit_peak(want, cv.ext.peak_db, vc.sr)
        moved = [not same(s, st[1]) for s in st[2:]]
        note(key, len(st) == 2 + len(h.parts) and same(st[0], want) and same(out, st[0]) and all(moved)
             and bool(torch.isfinite(st[0]).all()) and all(s.shape == st[1].shape for s in st) and not same(st[0], st[1]),
             f"{len(st)} stems of {tuple(st[1].shape)}; the parts differ from the lead: {moved}")
        return st
    st3 = mix_check("product/stems/mix-equals-numpy", conv, y_plain[0], H3)
    note("product/stems/lead-is-the-conversion-without-harmony", same(st3[1], y_plain[0]) and same(conv.convert([reqs[0]], stems=True)[0][0], y_plain[0])
         and same(conv.convert([reqs[0]], stems=True)[0][1], y_plain[0]))
    loud = serving.BatchConverter(vc, A, loudness_db=-20.0, peak_db=-6.0, **kw)
    stl = mix_check("product/stems/mix-with-loudness-and-ceiling", loud, None, H3)
    note("product/stems/per-voice-half-is-untouched-by-the-output-half", all(same(a, b) for a, b in zip(stl[1:], st3[1:])))
    y_sm = vc.special_match(files[0], ref, harmony=H3, **sk)
    y_cv = serving.BatchConverter(vc, serving.TargetVoice(vc, ref), **kw).convert([files[0]], harmony=H3)[0]
    note("product/special-match-goes-through-the-converter", same(y_sm, y_cv) and not same(y_sm, vc.special_match(files[0], ref, **sk)))

    # (c) the match stage: a part's features are the lead's, its f0 the oracle's on the lead's f0
    qx = vc.wavlm.encode_many([torch.from_numpy(reqs[0][0]).to(DEV)], max_batch=32, pow2_batches=True)[0]
    T = int(qx.shape[0])
    qf = dev(reqs[0][1][:T])
    pool = (A.feats, A.f0, A.harm, "mix", "post_opt_0.2")

    def f0_check(key, lead, part, p, extra=True):
        lh = lead[2].cpu().numpy()
        want, wt, _D, on, margin = HO.harmony(lh, [0, lh.size], [p])
        got = part[2].cpu().numpy()
        e = float((np.abs(got[on].astype(np.float64) - want[on].astype(np.float64)) / want[on].astype(np.float64)).max())
        WORST.append(e)
        keep = np.array_equal(got[~on].view(np.uint32), lh[~on].view(np.uint32))
        note(key, got.shape == want.shape and e <= REL_TOL and keep and margin >= MARGIN_MIN and int(on.sum()) > 20
             and same(part[0], lead[0]) and extra,
             f"{int(on.sum())} moved frames, rel {e:.2e}, others kept {keep}, margin {margin:.2e}; out_feats equal the lead's {same(part[0], lead[0])}")
        return wt

    p3 = HO.P("C:major", 2, 40.0)
    for name, more in (("none", dict(f0_shift="none")), ("median", {}), ("tune", dict(tune=Tuning("C:major", 1.0, 40.0)))):
        lead = M.match_features(qx, qf, *pool, pool_prep=A.prep, return_debug=True, **more)
        part = M.match_features(qx, qf, *pool, pool_prep=A.prep, return_debug=True, nn32=lead[3]["nn32"], harmony=shift(p3), **more)
        wt = f0_check(f"product/match/{name}/f0-equals-the-oracle", lead, part, p3,
                      lead[3]["harmony_notes"] is None and not same(lead[3]["idx_harm"], part[3]["idx_harm"])
                      and same(lead[3]["idx_wavlm"], part[3]["idx_wavlm"]) and same(lead[3]["tuned_notes"], part[3]["tuned_notes"]))
        note(f"product/match/{name}/debug-notes", np.array_equal(part[3]["harmony_notes"].cpu().numpy(), wt))
    pb = HO.P("A:minor", -2, 189.8)
    w37 = (0.3, 0.7)
    bl = M.match_features_blend([qx], [qf], [A, B], [w37], "mix", "post_opt_0.2", tune=["A:minor"])[0]
    bp = M.match_features_blend([qx], [qf], [A, B], [w37], "mix", "post_opt_0.2", tune=["A:minor"], harmony=[shift(pb)])[0]
    f0_check("product/match/blend/f0-equals-the-oracle", bl, bp, pb, not same(bl[1], bp[1]))
    dsec = (round(T * 1.25) * C.HOP + 0.5) / C.SAMPLE_RATE
    sx, sf = M.stretch_queries([qx], [qf], [dsec])
    ld = M.match_features(sx[0], sf[0], *pool, pool_prep=A.prep)
    pd = M.match_features(sx[0], sf[0], *pool, pool_prep=A.prep, harmony=shift(p3))
    f0_check("product/match/target-duration/f0-equals-the-oracle", ld, pd, p3, int(pd[2].shape[0]) == round(T * 1.25))
    yd = conv.convert([reqs[0]], harmony=H1, target_duration=dsec, stems=True)[0]
    note("product/match/target-duration/every-part-is-retimed", all(int(s.shape[0]) == round(T * 1.25) * C.HOP for s in yd) and len(yd) == 3)

    # (d) a mixed batch (no harmony, one part, three parts) on both routes == the single conversions
    hs = [None, H1, H3]
    alone = [conv.convert([r], harmony=h)[0].cpu() for r, h in zip(reqs, hs)]
    differs = [i for i in range(3) if not same(alone[i], y_plain[i])]
    note("product/converter/harmony-changes-the-output", differs == [1, 2], f"sources whose waveform differs from the default: {differs}")
    for route, rk in (("lanes", dict(match="lanes")), ("segmented", dict(match="segmented", match_batch=3))):
        cv = serving.BatchConverter(vc, A, **kw, **rk)
        ys = [y.cpu() for y in cv.convert(reqs, harmony=hs)]
        bad = [i for i in range(3) if not same(ys[i], alone[i])]
        cd = serving.BatchConverter(vc, A, harmony=H1, **kw, **rk)              # a default that is on: None takes it, "off" switches it off
        yd = [y.cpu() for y in cd.convert(reqs, harmony=["off", None, H3])]
        bad += [10 + i for i in range(3) if not same(yd[i], alone[i])]
        stems = cv.convert(reqs, harmony=hs, stems=True)
        bad += [20 + i for i in range(3) if not (len(stems[i]) == 2 + (0 if hs[i] is None else len(hs[i].parts)) and same(stems[i][0], alone[i])
                                                 and same(stems[i][1], y_plain[i]))]
        note(f"product/converter/{route}-batch-equals-single", not bad, f"sources that differ: {bad}")
    AB = serving.BatchConverter(vc, [A, B], blend=w37, **kw)
    sb = AB.convert([reqs[0]], harmony=H1, stems=True)[0]
    note("product/converter/blend", same(sb[1], AB.convert([reqs[0]])[0]) and not same(sb[2], sb[1])
         and x_equal(sb[0], HO.mix([s.cpu().numpy() for s in sb[1:]], H1.gains))[0])

    # (e) one encoder pass and one search per source and target voice, however many parts
    calls = dict(encode=0, rows=0)
    enc, knn = vc.wavlm.encode_many, ops.knn_topk

    def counting_encode(ws, **k):
        calls["encode"] += len(ws)
        return enc(ws, **k)

    def counting_knn(q, *a, **k):
        calls["rows"] += int(q.shape[0])
        return knn(q, *a, **k)
    vc.wavlm.encode_many, ops.knn_topk = counting_encode, counting_knn
    try:
        seen = []
        for cv, srcs, h in ((conv, [reqs[0]], H3), (AB, [reqs[0]], H3), (conv, reqs, hs),
                            (serving.BatchConverter(vc, A, match="segmented", **kw), reqs, [H3, H3, H3])):
            calls.update(encode=0, rows=0)
            cv.convert(srcs, harmony=h)
            frames = sum(M.frames_of(len(s[0]), vc.wavlm) for s in srcs) * (len(cv.voices) if cv.voices else 1)
            seen.append((calls["encode"], len(srcs), calls["rows"], frames))
    finally:
        vc.wavlm.encode_many, ops.knn_topk = enc, knn
    note("product/one-encoder-pass-and-one-search-per-source-and-voice", all(e == n and r == f for e, n, r, f in seen),
         f"(sources encoded, sources, query rows searched, frames x voices): {seen}")

    # (f) the queue: requests with different harmonies (and one without) share a batch; a bad one fails alone, at the door
    rq = serving.RequestQueue(conv, max_batch=3, max_wait_ms=5000.0)         # the batch closes when it is full: nothing waits
    try:
        errs = []
        for bad in (Harmony((2,)), "C:major", 2):
            try:
                rq.submit(reqs[0], harmony=bad)
            except ValueError as e:
                errs.append(e)
        futs = [rq.submit(reqs[1], harmony=H1), rq.submit(reqs[2], harmony=H3), rq.submit(reqs[0])]
        ys = [f.result(timeout=60) for f in futs]
    finally:
        rq.close()
    note("product/queue", len(errs) == 3 and rq.batches == [3] and rq.isolated == 0
         and same(ys[0], alone[1]) and same(ys[1], alone[2]) and same(ys[2], y_plain[0]), f"batches {rq.batches}; refused at the door: {errs}")

    # (g) bad values are refused before a file is read
    absent = os.path.join(tmp, "absent.wav")
    nref = 0
    for bad in (Harmony((2,)), "C:major", 3):
        for fn in (lambda: vc.special_match(absent, absent, harmony=bad), lambda: conv.convert([absent], harmony=bad),
                   lambda: vc.many_to_one([absent], absent, target=A, harmony=bad), lambda: conv.convert_files([absent], harmony=bad)):
            try:
                fn()
            except ValueError:
                nref += 1
    note("product/refusals", nref == 12, f"{nref} of 12 refused with ValueError")
    note("product/largest-oracle-error", max(WORST) <= REL_TOL, f"{max(WORST):.3e}")


if __name__ == "__main__":
    sys.exit(run_cases([("kernel", case_kernel), ("mix", case_mix), ("product", case_product)], sys.argv[1]))
