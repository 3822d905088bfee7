"""Child interpreter of tests/test_gpu_tune.py: runs every pitch-correction case on the GPU and writes a JSON report
{check name: {"ok": bool, "detail": str}}; the pytest process only reads it (it must not initialise the GPU itself).

    python tests/tune_child.py REPORT.json

The reference is tests/tune_oracle.py fed the DEVICE's shifted f0 (the shift has its own tests; what is judged here is the
correction).  Tolerances, none taken from what the kernel gives:
  notes            exactly equal: tests/test_tune_cpu.py shows that every kernel case stands >= 1e-6 semitone from every note
                   decision going the other way, the product cases check the same here on the device's f0 before they compare,
                   and an ulp of the device's fp64 log moves a pitch by 1e-13
  unpitched frames bit-equal to the input
  pitched f0       largest relative error <= 5e-6, tests/pitch_child.py's bound for this stage's log / exp (the one-pole is a
                   contraction, so an input difference does not grow; what remains is the final fp32 rounding)
  hard snap        every pitched output within the same 5e-6 of tuning_hz * 2^((note - 69) / 12): no oracle f0 involved
Everything else is bit equality."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np
import torch

import pitch_oracle as P
import tune_oracle as O
from knn_svc_amd import config as C, matching as M, ops
from knn_svc_amd.options import TUNE_OFF, Tuning
from tests.gpu_child import DEV, dev, guarded, misaligned, note, run_cases, same, table, tiny_vc, write_clip

REL_TOL = 5e-6
MARGIN_MIN = 1e-6
WORST = []


def tuning(t):
    """The oracle's tuning as the options.Tuning the code under test takes."""
    return None if t is None else Tuning(*t.spec)


def against_oracle(f0_host, seg, tunings, got, got_notes):
    """-> (ok, detail): notes exactly, unpitched frames bit for bit, pitched f0 within REL_TOL; the oracle's margin is part of
    the verdict (a case closer than MARGIN_MIN to a decision may not be compared exactly)."""
    want, wn, margin = O.tune(f0_host, seg, tunings)
    got, gn = got.cpu().numpy(), got_notes.cpu().numpy()
    if got.shape != want.shape or gn.shape != wn.shape or gn.dtype != np.int32:
        return False, f"shapes {got.shape} {gn.shape} {gn.dtype}"
    on = wn >= 0
    notes_bad = int((gn != wn).sum())
    keep = np.array_equal(got[~on].view(np.uint32), np.asarray(f0_host, np.float32)[~on].view(np.uint32))
    e = float((np.abs(got[on].astype(np.float64) - want[on].astype(np.float64)) / want[on].astype(np.float64)).max()) if on.any() else 0.0
    WORST.append(e)
    return (notes_bad == 0 and keep and e <= REL_TOL and margin >= MARGIN_MIN,
            f"{int(on.sum())} corrected frames; notes that differ {notes_bad}; others kept {keep}; rel {e:.2e}; margin {margin:.2e}")


# ------------------------------------------------------------------ 1. the kernel
def case_kernel():
    cases = O.kernel_cases()
    # (a) edges: one stacked table, output into guarded rows, input one float off a 16-byte boundary
    f0h, seg, tun, why = O.edges()
    tn = [tuning(t) for t in tun]
    f0 = misaligned(f0h)
    out, untouched = guarded(f0h.size)
    got, notes = ops.tune_f0_seg(f0, seg, tn, return_notes=True)
    ok, detail = against_oracle(f0h, seg, tun, got, notes)
    note("kernel/edges/equals-the-oracle", ok, detail)
    # the library call itself, writing into guarded rows of f0 and of notes
    from knn_svc_amd import _lib
    import ctypes
    lib = _lib.load()
    n = len(seg) - 1
    nbuf = torch.full((f0h.size + 128,), -77, device=DEV, dtype=torch.int32)
    ws_bytes = lib.knnsvc_tune_f0_workspace_bytes(f0h.size, n)
    ws = torch.full((ws_bytes + 512,), 0x5A, device=DEV, dtype=torch.uint8)
    live = [t if t is not None else TUNE_OFF for t in tn]
    out.fill_(-7.25e11)
    rc = lib.knnsvc_tune_f0_seg(f0.data_ptr(), (ctypes.c_int64 * (n + 1))(*seg), n, (ctypes.c_int32 * n)(*[t.mask if t.on else 0 for t in live]),
                                (ctypes.c_double * n)(*[t.strength for t in live]), (ctypes.c_double * n)(*[t.alpha for t in live]),
                                (ctypes.c_double * n)(*[t.log_ref for t in live]), out.data_ptr(), nbuf[64:].data_ptr(), ws[256:].data_ptr(),
                                ws_bytes, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    note("kernel/edges/guards-untouched", rc == 0 and untouched() and same(out, got) and same(nbuf[64:64 + f0h.size], notes)
         and bool((nbuf[:64] == -77).all()) and bool((nbuf[64 + f0h.size:] == -77).all())
         and bool((ws[:256] == 0x5A).all()) and bool((ws[256 + ws_bytes:] == 0x5A).all()),
         f"rc {rc}; workspace {ws_bytes} bytes for {f0h.size} frames")
    off_s = tun.index(None)
    a, b = seg[off_s], seg[off_s + 1]
    note("kernel/edges/off-segment-keeps-its-bits", same(got[a:b], f0[a:b]) and bool((notes[a:b] == -1).all()), why[off_s])
    bad = []
    for s in range(n):
        a, b = seg[s], seg[s + 1]
        if tn[s] is None:
            continue
        y1, n1 = ops.tune_f0_seg(f0[a:b].contiguous(), [0, b - a], [tn[s]], return_notes=True)
        if not (same(y1, got[a:b]) and same(n1, notes[a:b])):
            bad.append(s)
    note("kernel/edges/each-segment-alone-is-bit-identical", not bad, f"segments that differ: {bad}")
    again, notes2 = ops.tune_f0_seg(f0, seg, tn, return_notes=True)
    note("kernel/edges/second-call-is-bit-identical", same(again, got) and same(notes2, notes) and same(ops.tune_f0_seg(f0, seg, tn), got))

    # (b) the melodies, the stepwise melody and the long run: per case ONE call, the source stacked once per setting
    for name in ("up", "up-shifted", "down", "down-shifted", "near", "near-shifted", "steps", "one-run"):
        f0h, seg, tun = cases[name]
        got, notes = ops.tune_f0_seg(dev(f0h), seg, [tuning(t) for t in tun], return_notes=True)
        ok, detail = against_oracle(f0h, seg, tun, got, notes)
        note(f"kernel/{name}/equals-the-oracle", ok, f"{len(tun)} settings x {seg[1]} frames; " + detail)
        # hard snap: the settings with strength 1 and retune 0 land on the grid, judged without the oracle's f0
        g, nn = got.cpu().numpy().astype(np.float64), notes.cpu().numpy()
        worst, cnt = 0.0, 0
        for s, t in enumerate(tun):
            if t.spec[1] == 1.0 and t.spec[2] == 0.0:
                a, b = seg[s], seg[s + 1]
                on = nn[a:b] >= 0
                grid = O.grid_hz(nn[a:b][on], t.spec[3])
                worst = max(worst, float((np.abs(g[a:b][on] - grid) / grid).max()))
                cnt += int(on.sum())
        note(f"kernel/{name}/hard-snap-lands-on-the-grid", cnt > 0 and worst <= REL_TOL, f"{cnt} frames, rel {worst:.2e}")
    note("kernel/largest-oracle-error", max(WORST) <= REL_TOL, f"{max(WORST):.3e}")

    # (c) seventy segments, mixed on / off / scales, one ops call (two library calls) == each segment alone
    rng = np.random.default_rng(70)
    lens = [int(v) for v in rng.integers(1, 48, size=70)]
    lens[5], lens[64], lens[69] = 300, 1100, 1                    # more than 1024 frames in a segment of the second call; a 1-frame tail
    tr = P.track(sum(lens), 150.0, 71)
    f0 = dev(tr); seg = table(lens)
    pick = [None, TUNE_OFF, Tuning("chromatic"), Tuning("C:major", 1.0, 0.0), Tuning("G:major", 0.6, 200.0), Tuning(O.CUSTOM, 0.8, 40.0, 432.0)]
    tn = [pick[int(v)] for v in rng.integers(0, len(pick), size=70)]
    tn[64], tn[69] = pick[4], pick[2]
    got, notes = ops.tune_f0_seg(f0, seg, tn, return_notes=True)
    bad = []
    for i in range(70):
        a, b = seg[i], seg[i + 1]
        y1, n1 = ops.tune_f0_seg(f0[a:b].contiguous(), [0, b - a], [tn[i]], return_notes=True)
        if n1 is None:                                     # off alone: the input itself, no notes
            okk = y1.data_ptr() == f0[a:b].data_ptr() and same(got[a:b], f0[a:b]) and bool((notes[a:b] == -1).all())
        else:
            okk = same(got[a:b], y1) and same(notes[a:b], n1)
        if not okk:
            bad.append(i)
    kinds = len({id(t) for t in tn})
    note("kernel/seventy-segments-equal-each-alone", not bad and kinds == len(pick), f"segments that differ: {bad}; {kinds} kinds of setting")
    # a run of 64 segments that is all off is copied, not launched; all off: the input object
    half = [None] * 64 + tn[64:]
    g2, n2 = ops.tune_f0_seg(f0, seg, half, return_notes=True)
    note("kernel/all-off-chunk-is-copied", same(g2[:seg[64]], f0[:seg[64]]) and bool((n2[:seg[64]] == -1).all())
         and same(g2[seg[64]:], got[seg[64]:]) and same(n2[seg[64]:], notes[seg[64]:]))
    y0 = ops.tune_f0_seg(f0, seg, [None, TUNE_OFF] * 35)
    y1, n1 = ops.tune_f0_seg(f0, seg, [None] * 70, return_notes=True)
    note("kernel/all-off-returns-the-input-object", y0 is f0 and y1 is f0 and n1 is None)

    # (d) refusals through ops
    refused = 0
    t = Tuning("chromatic")
    for args in ((f0, seg, [t] * 69), (f0.to(torch.int32), seg, [t] * 70), (f0[:100].contiguous(), seg, [t] * 70)):
        try:
            ops.tune_f0_seg(*args)
        except ops.KnnSvcError:
            refused += 1
    note("kernel/ops-refuses", refused == 3, f"{refused} of 3 refused")


# ------------------------------------------------------------------ 2. product
def sharp_track(n_frames, seed, base=52):
    """A stepwise melody written 35 cents sharp (5 cents of seeded noise), notes of 20 frames, a 5-frame rest after every third."""
    rng = np.random.default_rng(seed)
    parts, k = [], 0
    while sum(p.size for p in parts) < n_frames:
        parts.append(O.hz(base + int(rng.integers(0, 13)) + 0.35 + 0.05 * rng.uniform(-1, 1, 20)))
        k += 1
        if k % 3 == 0:
            parts.append(np.zeros(5, np.float32))
    return np.concatenate(parts)[:n_frames].copy()


def case_product(tmp):
    from knn_svc_amd import serving
    pools = {}
    for name, hz, seed in (("A", 233.0, 900), ("B", 147.0, 910)):
        pools[name] = os.path.join(tmp, name); os.makedirs(pools[name])
        for i in range(2):
            n = 3 * 16000 + 37 * i
            write_clip(os.path.join(pools[name], f"t{i}.wav"), n, seed + i, f0=P.track(n // 320 + 1, hz, seed + 40 + i))
    reqs, files = [], []
    for i, n in enumerate([16000 * 2 + 11, 9000, 16000 + 641, 16000 + 2000]):
        f = sharp_track(n // 320 + 1, 50 + i)
        p = os.path.join(tmp, f"s{i}.wav")
        write_clip(p, n, 700 + i, f0=f)
        files.append(p); reqs.append((M.load_utterance(p)[0], f))
    vc = tiny_vc()
    src, pool = files[0], pools["A"]
    kw = dict(ckpt_type="mix", post_opt="post_opt_0.2")
    mk = dict(prioritize_f0=True, **kw)
    mi = lambda **k: M.match_at_inference_time(src, pool, vc.wavlm, vc.weighting, vc.weighting, tgt_dataset_path=pool, **mk, **k)

    def f0_check(key, untuned, tuned, t):
        """``tuned`` (device f0) against the oracle applied to ``untuned`` (device f0) with the oracle's tuning ``t``."""
        uh = untuned.cpu().numpy()
        want, wn, margin = O.tune(uh, [0, uh.size], [t])
        got = tuned.cpu().numpy()
        on = wn >= 0
        e = float((np.abs(got[on].astype(np.float64) - want[on].astype(np.float64)) / want[on].astype(np.float64)).max())
        WORST.append(e)
        keep = np.array_equal(got[~on].view(np.uint32), uh[~on].view(np.uint32))
        moved = float(np.abs(got[on] / uh[on] - 1).max())
        note(key, got.shape == want.shape and e <= REL_TOL and keep and margin >= MARGIN_MIN and int(on.sum()) > 20 and moved > 1e-3,
             f"{int(on.sum())} corrected frames, rel {e:.2e}, others kept {keep}, margin {margin:.2e}, largest correction {moved:.3f}")

    # (a) defaults, explicit None and "off": the same bits everywhere
    of0, hw0, _a, sf0 = mi()
    of1, hw1, _a, sf1 = mi(tune=None)
    of2, hw2, _a, sf2 = mi(tune="off")
    sk = dict(save=False, **kw)
    ref = os.path.join(pool, "t0.wav")
    y0 = vc.special_match(src, ref, **sk)
    y1 = vc.special_match(src, ref, tune=None, **sk)
    eq = [same(a[src], b[src]) for a, b in ((of0, of1), (hw0, hw1), (sf0, sf1), (of0, of2), (hw0, hw2), (sf0, sf2))] + [same(y0, y1)]
    note("product/defaults-are-bit-identical", all(eq), f"features, harmonics, shifted f0 (x2), waveform: {eq}")

    # (b) f0_shift="none" with a key: the f0 equals the oracle on the untuned conversion's f0, the waveform differs
    cmaj = O.T("C:major")
    _o, _h, _a, sfn = mi(f0_shift="none")
    ot, _h, _a, sft = mi(f0_shift="none", tune="C:major")
    f0_check("product/none-with-a-key/f0-equals-the-oracle", sfn[src], sft[src], cmaj)
    yn = vc.special_match(src, ref, f0_shift="none", **sk)
    yt = vc.special_match(src, ref, f0_shift="none", tune="C:major", **sk)
    yt2 = vc.special_match(src, ref, f0_shift="none", tune=Tuning("C:major"), **sk)
    d = float((yt - yn).abs().max())
    note("product/none-with-a-key/changes-the-waveform", d > 0 and bool(torch.isfinite(yt).all()) and yt.shape == yn.shape and same(yt, yt2),
         f"max |tuned - untuned| {d:.2e}")
    # the median shift (an arbitrary interval) with a key, and the notes of the debug dict
    _o, _h, _a, sfm = mi(tune=Tuning("G:major", 0.6, 200.0))
    f0_check("product/median-with-a-key/f0-equals-the-oracle", sf0[src], sfm[src], O.T("G:major", 0.6, 200.0))
    vc.wavlm.set_layer_mix(M._mix_of(vc.weighting, vc.wavlm))
    A, B = (serving.TargetVoice(vc, pools[k]) for k in "AB")
    qx = vc.wavlm.encode_many([torch.from_numpy(reqs[0][0]).to(DEV)], max_batch=32, pow2_batches=True)[0]
    T = int(qx.shape[0])
    qf = dev(reqs[0][1][:T])
    plain = M.match_features(qx, qf, A.feats, A.f0, A.harm, "mix", "post_opt_0.2", pool_prep=A.prep, return_debug=True)
    tuned = M.match_features(qx, qf, A.feats, A.f0, A.harm, "mix", "post_opt_0.2", pool_prep=A.prep, return_debug=True, tune="chromatic")
    _w, wn, margin = O.tune(plain[2].cpu().numpy(), [0, T], [O.T("chromatic")])
    note("product/debug-dict", plain[3]["tuned_notes"] is None and margin >= MARGIN_MIN
         and np.array_equal(tuned[3]["tuned_notes"].cpu().numpy(), wn) and same(plain[3]["shift_semitones"], tuned[3]["shift_semitones"])
         and not same(plain[3]["idx_harm"], tuned[3]["idx_harm"]) and same(plain[3]["idx_wavlm"], tuned[3]["idx_wavlm"]),
         f"notes equal the oracle's; margin {margin:.2e}; the pitched selection moved, the unpitched one did not")

    # (c) a batch of four settings on both match routes == the four single conversions
    sets = ["off", "chromatic", "A:minor", Tuning("E:blues", strength=0.5)]
    conv = serving.BatchConverter(vc, A, **kw)
    alone = [serving.BatchConverter(vc, A, tune=None if t == "off" else t, **kw).convert([r])[0].cpu() for r, t in zip(reqs, sets)]
    plain4 = [conv.convert([r])[0].cpu() for r in reqs]
    movedi = [i for i in range(4) if not same(alone[i], plain4[i])]
    note("product/converter/settings-change-the-output", movedi == [1, 2, 3], f"sources whose waveform differs from the default: {movedi}")
    for route, rk in (("lanes", dict(match="lanes")), ("segmented", dict(match="segmented", match_batch=3))):
        cv = serving.BatchConverter(vc, A, **kw, **rk)
        ys4 = [y.cpu() for y in cv.convert(reqs, tune=sets)]
        bad = [i for i in range(4) if not same(ys4[i], alone[i])]
        # a converter whose default is on: None entries take it, "off" switches it off
        cd = serving.BatchConverter(vc, A, tune="chromatic", **kw, **rk)
        ys4d = [y.cpu() for y in cd.convert(reqs, tune=["off", None, "A:minor", sets[3]])]
        bad += [10 + i for i in range(4) if not same(ys4d[i], alone[i])]
        note(f"product/converter/{route}-batch-equals-single", not bad, f"sources that differ: {bad}")

    # (d) a blend of two voices with a key == the oracle on the blend's untuned f0
    w37 = (0.3, 0.7)
    bu = M.match_features_blend([qx], [qf], [A, B], [w37], "mix", "post_opt_0.2")[0]
    bt = M.match_features_blend([qx], [qf], [A, B], [w37], "mix", "post_opt_0.2", tune=["A:minor"])[0]
    f0_check("product/blend/f0-equals-the-oracle", bu[2], bt[2], O.T("A:minor"))
    AB = serving.BatchConverter(vc, [A, B], blend=w37, **kw)
    yb, ybt = AB.convert([reqs[0]])[0].cpu(), AB.convert([reqs[0]], tune="A:minor")[0].cpu()
    note("product/blend/changes-the-waveform", not same(yb, ybt) and yb.shape == ybt.shape and same(bu[0], bt[0]) and not same(bu[1], bt[1]),
         f"max |tuned - untuned| {float((yb - ybt).abs().max()):.2e}; the blended harmonics moved, the blended features did not")

    # (e) target_duration with a key == the oracle on the re-timed, shifted f0
    dsec = (round(T * 1.25) * C.HOP + 0.5) / C.SAMPLE_RATE
    _o, _h, _a, sfd = mi(target_duration=dsec)
    odt, _h, _a, sfdt = mi(target_duration=dsec, tune=Tuning("C:major", 1.0, 40.0))
    f0_check("product/with-target-duration/f0-equals-the-oracle", sfd[src], sfdt[src], O.T("C:major", 1.0, 40.0))
    note("product/with-target-duration/length", int(sfdt[src].shape[0]) == round(T * 1.25) == int(odt[src].shape[0]), f"T {T} -> {int(sfdt[src].shape[0])}")

    # (f) the queue: two requests with different scales (and one without) share a batch; a bad one fails alone, at the door
    rq = serving.RequestQueue(conv, max_batch=3, max_wait_ms=5000.0)         # the batch closes when it is full: nothing waits
    try:
        err = None
        try:
            rq.submit(reqs[0], tune="H:major")
        except ValueError as e:
            err = e
        futs = [rq.submit(reqs[1], tune="chromatic"), rq.submit(reqs[2], tune="A:minor"), rq.submit(reqs[0])]
        ys = [f.result(timeout=60) for f in futs]
    finally:
        rq.close()
    note("product/queue", isinstance(err, ValueError) and rq.batches == [3] and rq.isolated == 0
         and same(ys[0], alone[1]) and same(ys[1], alone[2]) and same(ys[2], plain4[0]), f"batches {rq.batches}; refused at the door: {err}")

    # (g) bad values are refused before a file is read
    absent = os.path.join(tmp, "absent.wav")
    nref = 0
    for bad in ("H:major", "C:000000000000", 3):
        for fn in (lambda: vc.special_match(absent, absent, tune=bad), lambda: conv.convert([absent], tune=bad),
                   lambda: vc.many_to_one([absent], absent, target=A, tune=bad), lambda: vc.bulk_match(absent, absent, absent, tune=bad)):
            try:
                fn()
            except ValueError:
                nref += 1
    note("product/refusals", nref == 12, f"{nref} of 12 refused with ValueError")
    note("product/largest-oracle-error", max(WORST) <= REL_TOL, f"{max(WORST):.3e}")


if __name__ == "__main__":
    sys.exit(run_cases([("kernel", case_kernel), ("product", case_product)], sys.argv[1]))
