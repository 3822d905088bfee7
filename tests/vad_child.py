"""Child interpreter of tests/test_gpu_vad.py: runs every trimmer case on the GPU and writes a JSON report
{check name: {"ok": bool, "detail": str}}; the pytest process only reads it (it must not initialise the GPU itself).

    python tests/vad_child.py REPORT.json

The reference is tests/vad_oracle.py (fp64 numpy), the inputs are tests/vad_cases.py.  Tolerances, none of them taken from what the
kernels give:
  cut points    equal to the oracle's, exactly; every case first has to stand, by the oracle alone, at least 1e-6 off every decision
                of the scan (vad_cases.MARGIN; tests/test_vad_cpu.py shows the same without a GPU)
  measures      within 1e-6 of the oracle's — the margin inside which no decision can flip (fp64 on both sides: rounding stays far
                below it); the exact zeros are the same entries
Everything else is bit equality."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np
import torch

import vad_cases as VC
import vad_oracle as O
from knn_svc_amd import audio_io, ops, synthetic as S
from tests.gpu_child import DEV, note, run_cases, tiny_vc, write_clip

TOL = 1e-6


def refused(fn):
    try:
        fn()
    except ops.KnnSvcError:
        return True
    return False


def on_device(x, level, sr=16000):
    """-> ((lstrip, rstrip), forward measures, reversed measures) of one recording in a call of its own."""
    strip, meas = ops.vad_trim([torch.from_numpy(x).to(DEV)], level, sample_rate=sr, return_measures=True)
    return tuple(int(v) for v in strip[0].cpu()), meas[0][0].cpu().numpy(), meas[0][1].cpu().numpy()


def compare(name, got, want, info, worst):
    """One recording against the oracle: a cut/ and a measures/ entry."""
    if info["margin"] < VC.MARGIN:
        note(f"cut/{name}", False, f"precondition: a decision stands {info['margin']:.3g} from flipping; choose another seed or level")
        return
    note(f"cut/{name}", got[0] == want, f"device {got[0]} / oracle {want}, margin {info['margin']:.3g}")
    errs, same_zeros, shapes = [], True, True
    for g, w in ((got[1], info["fwd"]), (got[2], info["rev"])):
        shapes = shapes and g.shape == w.shape and g.dtype == np.float64
        if shapes and w.size:
            errs.append(float(np.abs(g - w).max()))
            same_zeros = same_zeros and np.array_equal(g == 0.0, w == 0.0)
    err = max(errs, default=0.0)
    worst.append(err)
    note(f"measures/{name}", shapes and err <= TOL and same_zeros,
         f"{info['fwd'].size} measurements per direction, largest |device - oracle| {err:.3e}, same zeros {same_zeros}")


# ------------------------------------------------------------------ 1. kernels against the oracle
def case_oracle():
    cases = VC.cases()
    device, worst = {}, []
    for name, (x, level) in cases.items():
        want, info = O.trim(x, level, details=True)
        device[name] = on_device(x, level)
        compare(name, device[name], want, info, worst)
    x, level, sr = VC.tone_8k()
    want, info = O.trim(x, level, sr, details=True)
    compare("tone-8k", on_device(x, level, sr), want, info, worst)
    print(f"largest |measure - oracle| over all cases: {max(worst):.3e}", flush=True)
    note("measures/largest-error", max(worst) <= TOL, f"{max(worst):.3e}")
    # the call without measures
    x, level = cases["two-bursts/gap8"]
    strip = ops.vad_trim(torch.from_numpy(x).to(DEV), level)
    note("cut/plain-call", strip.shape == (1, 2) and strip.dtype == torch.int64 and strip.is_cuda
         and tuple(strip[0].tolist()) == device["two-bursts/gap8"][0], f"{strip.tolist()}")
    # five recordings of different lengths, a dropped one among them, in ONE call
    names = ["tone2s/7", "n1599", "golden-tgt", "short-voiced", "two-bursts/gap3"]
    assert len({cases[n][0].size for n in names}) == 5 and {cases[n][1] for n in names} == {7.0}
    strip, meas = ops.vad_trim([torch.from_numpy(cases[n][0]).to(DEV) for n in names], 7.0, return_measures=True)
    strip = strip.cpu().tolist()
    for i, n in enumerate(names):
        same = (tuple(strip[i]) == device[n][0] and np.array_equal(meas[i][0].cpu().numpy(), device[n][1])
                and np.array_equal(meas[i][1].cpu().numpy(), device[n][2]))
        note(f"stacked/{n}", same, f"{strip[i]} / alone {device[n][0]}")
    # refusals with device tensors
    z = torch.zeros(8000, device=DEV)
    bad = [lvl for lvl in (0, -3, float("nan"), float("inf")) if not refused(lambda: ops.vad_trim(z, lvl))]
    note("refuse/levels", not bad, f"accepted: {bad}")
    note("refuse/shape", refused(lambda: ops.vad_trim(torch.zeros(2, 8000, device=DEV), 7)))
    note("refuse/rate", refused(lambda: ops.vad_trim(z, 7, sample_rate=48000)))


# ------------------------------------------------------------------ 2. product
def case_product(tmp):
    """A target whose recording starts and ends with 1 s of digital silence plus faint noise, one source, the small models."""
    from knn_svc_amd import matching, serving
    quiet = lambda seed: (1e-4 * np.random.default_rng(seed).standard_normal(16000)).astype(np.float32)
    w, _f = S.synth_clip(2 * 16000 + 123, seed=900)
    tgt = os.path.join(tmp, "tgt.wav")
    audio_io.write_wav_pcm16(tgt, np.concatenate([quiet(1), w, quiet(2)]), 16000)
    np.save(tgt[:-4] + "_f0.npy", (150.0 + np.arange((4 * 16000 + 123) // 320 + 1)).astype(np.float32))     # every frame its own value
    src = os.path.join(tmp, "src.wav")
    write_clip(src, 16000 + 641, 700, f0_mul=1.2)
    vc = tiny_vc()
    vc.wavlm.set_layer_mix(matching._mix_of(vc.weighting, vc.wavlm))
    whole = matching.get_complete_spk_pool(tgt, vc.wavlm, vad_trigger_level=0)
    cut = matching.get_complete_spk_pool(tgt, vc.wavlm, vad_trigger_level=7)
    n_whole, n_cut = whole[0][tgt].shape[0], cut[0][tgt].shape[0]
    note("product/pool/fewer-frames", n_cut < n_whole, f"{n_cut} frames at level 7, {n_whole} at level 0")
    # the pool of the hand-trimmed waveform (cut points from the oracle)
    x, f0 = matching.load_utterance(tgt)
    (l, r), d = O.trim(x, 7.0, details=True)
    note("product/pool/precondition", d["margin"] >= VC.MARGIN and l >= 12800 and r >= 12800,
         f"oracle cuts {(l, r)} (most of each silent second goes), margin {d['margin']:.3g}")
    hand = torch.from_numpy(np.ascontiguousarray(x[l:len(x) - r])).to(DEV)
    feats = vc.wavlm.encode_many([hand], pow2_batches=True)[0]
    T = feats.shape[0]
    _f0, harm_want, spec_want = matching.side_features_many([hand], [f0[l // 320:l // 320 + T + 1]], [T])[0]
    matching_pool, synth, _audio, specs, f0p, harmp = cut
    note("product/pool/features-of-the-hand-trimmed-waveform",
         list(matching_pool) == [tgt] and T == matching.frames_of(len(x) - l - r, vc.wavlm)
         and torch.equal(matching_pool[tgt], feats) and torch.equal(synth[tgt], feats)
         and torch.equal(specs[tgt], spec_want) and torch.equal(harmp[tgt], harm_want), f"{T} frames")
    note("product/pool/f0-is-the-sliced-track",
         torch.equal(f0p[tgt].cpu(), torch.from_numpy(f0[l // 320:l // 320 + T])) and float(f0p[tgt][0]) == 150.0 + l // 320,
         f"first value {float(f0p[tgt][0])}, lstrip / 320 = {l // 320}")
    # a pool without speech
    p = os.path.join(tmp, "quiet.wav")
    audio_io.write_wav_pcm16(p, (1e-4 * np.random.default_rng(5).standard_normal(32000)).astype(np.float32), 16000)
    np.save(p[:-4] + "_f0.npy", np.zeros(101, np.float32))
    try:
        matching.get_complete_spk_pool(p, vc.wavlm, vad_trigger_level=7)
        note("product/pool/empty-pool-refused", False, "no error")
    except ops.KnnSvcError as e:
        note("product/pool/empty-pool-refused", "left no file" in str(e), str(e))
    # special_match: the switch, and the level without the switch
    kw = dict(ckpt_type="mix", post_opt="post_opt_0.2", save=False)
    off = vc.special_match(src, tgt, **kw)
    off3 = vc.special_match(src, tgt, vad_trigger_level=3, **kw)
    off12 = vc.special_match(src, tgt, use_vad=False, vad_trigger_level=12, **kw)
    note("product/special_match/switch-off-ignores-the-level", torch.equal(off, off3) and torch.equal(off, off12))
    on = vc.special_match(src, tgt, use_vad=True, **kw)
    note("product/special_match/source-length", on.shape == off.shape and bool(torch.isfinite(on).all()) and not torch.equal(on, off),
         f"{tuple(on.shape)} / {tuple(off.shape)}")
    note("product/target-voice", serving.TargetVoice(vc, tgt, vad_trigger_level=7).frames == n_cut
         and serving.TargetVoice(vc, tgt).frames == n_whole)


if __name__ == "__main__":
    sys.exit(run_cases([("oracle", case_oracle), ("product", case_product)], sys.argv[1]))
