"""Child interpreter of tests/test_gpu_loudness.py: runs every loudness case on the GPU and writes a JSON report
{check name: {"ok": bool, "detail": str}}; the pytest process only reads it (it must not initialise the GPU itself).

    python tests/loudness_child.py REPORT.json

The reference is tests/loudness_oracle.py (fp64 numpy).  Tolerances, none of them taken from what the kernels give:
  lkfs against the oracle   1e-4 dB absolute (the result is fp32 rounded from fp64 arithmetic: one ulp at 70 is 7.6e-6), counts equal;
                            every input first has to stand, by the oracle, at least 0.01 dB off both gate thresholds in every
                            block, so that a gate decision cannot hide an error
  gain                      out == x * g to rtol 2e-6 with g recomputed on the host from the returned lkfs; the oracle's loudness
                            of out within 3e-4 dB of the target (1e-4 measurement + 1e-4 re-measurement + fp32 rounding of g)
  files                     within 1e-3 dB of the target by the oracle on the samples read back
Everything else is bit equality."""
import ctypes
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np
import torch

import loudness_oracle as O
from knn_svc_amd import _lib, audio_io, ops
from tests.gpu_child import DEV, misaligned, note, run_cases, same, tiny_vc, write_clip

TOL_DB = 1e-4
MARGIN_DB = 0.01


def close_db(got, want, tol):
    if math.isinf(want) or math.isinf(got) or math.isnan(got):
        return got == want
    return abs(got - want) <= tol


def noise(n, seed):
    return (0.2 * np.random.default_rng(seed).standard_normal(n)).astype(np.float32)


def long_clip():
    """30 s: a tone gliding 150 -> 600 Hz under a slow envelope (0.02 .. 0.5, so the relative gate drops blocks), plus noise."""
    n = 480000
    t = np.arange(n) / 16000.0
    phase = 2 * np.pi * (150.0 * t + 0.5 * (450.0 / 30.0) * t * t)
    env = 0.26 + 0.24 * np.sin(2 * np.pi * 0.11 * t + 0.3)
    return (env * np.sin(phase) + 0.004 * np.random.default_rng(12).standard_normal(n)).astype(np.float32)


_ORACLE = {}


def oracle(name, x, sr):
    """(lkfs, counts, margin) of a named input, computed once and shared."""
    if name not in _ORACLE:
        _ORACLE[name] = O.loudness(x, sr, details=True)
    return _ORACLE[name]


def measure(xg, sr=16000):
    lk, cn = ops.loudness(xg, sr, return_counts=True)
    return float(lk), tuple(int(v) for v in cn.cpu())


# ------------------------------------------------------------------ 1. kernel against oracle
def inputs_16k():
    Cn, W = ops.loudness_layout()
    pad = lambda v: v if v >= 6400 else v + 6400          # a length that tests a chunk edge still has to hold one block
    cases = [(f"noise{n}", noise(n, 100 + n)) for n in (0, 1, 6399, 6400, 7999, 8000, 8001)]
    cases += [(f"edge{tag}-{pad(v)}", noise(pad(v), 200 + i)) for i, (tag, v) in enumerate(
        (("C-1", Cn - 1), ("C", Cn), ("C+1", Cn + 1), ("W-1", W - 1), ("W", W), ("W+1", W + 1), ("3W+C+1", 3 * W + Cn + 1)))]
    imp = np.zeros(8000, np.float32)
    imp[0] = 1.0
    cases += [("impulse", imp), ("constant", np.full(16000, 0.5, np.float32)), ("gated", O.gated_signal()), ("clip30s", long_clip())]
    return cases


# other rates: 48 kHz (steps of 75 chunks), and two whose 100 ms step is NO multiple of the chunk length, so that chunks straddle
# step boundaries and a chunk's energy is split between two steps (44.1 kHz: step 4410 = 68 chunks + 58; 24 kHz: 2400 = 37 chunks
# + 32); both lengths end in the middle of a step and of a chunk
OTHER_RATES = [("48k-96005", 48000, 96005, 48), ("44k1-56445", 44100, 56445, 44), ("24k-30011", 24000, 30011, 24)]


def case_oracle():
    Cn, _W = ops.loudness_layout()
    for name, sr, n, _seed in OTHER_RATES[1:]:
        assert (sr // 10) % Cn and n % (sr // 10) and n % Cn, (name, "no longer straddles: choose another rate / length")
    rates = {name: sr for name, sr, _n, _seed in OTHER_RATES}
    for name, x in inputs_16k() + [(name, noise(n, seed)) for name, _sr, n, seed in OTHER_RATES]:
        sr = rates.get(name, 16000)
        want, wcounts, margin = oracle(name, x, sr)
        if margin < MARGIN_DB:
            note(f"oracle/{name}", False, f"precondition: a block stands {margin:.4f} dB from a gate threshold; choose another seed")
            continue
        got, gcounts = measure(torch.from_numpy(x).to(DEV), sr)
        note(f"oracle/{name}", close_db(got, want, TOL_DB) and gcounts == wcounts,
             f"n {x.size}: lkfs {got!r} / oracle {want!r}, counts {gcounts} / {wcounts}, gate margin {margin:.3f} dB")
    lib = _lib.load()
    name, x = "gated", O.gated_signal()
    want, wcounts, _ = oracle(name, x, 16000)
    # counts = NULL
    xg = torch.from_numpy(x).to(DEV)
    note("oracle/counts-null", close_db(float(ops.loudness(xg)), want, TOL_DB), "")
    # a waveform that starts 4 bytes off a 16-byte boundary
    view = misaligned(x)
    got, gcounts = measure(view)
    note("oracle/wav-4-bytes-off-alignment", view.data_ptr() % 16 == 4 and close_db(got, want, TOL_DB) and gcounts == wcounts,
         f"pointer % 16 = {view.data_ptr() % 16}, lkfs {got!r} / {want!r}, counts {gcounts}")
    # a workspace of exactly the reported size between sentinel bytes
    for nm, xs in (("gated", x), ("edgeW+1", noise(ops.loudness_layout()[1] + 1, 205))):
        w0, c0, _ = oracle(nm + "/ws", xs, 16000)
        need = lib.knnsvc_loudness_workspace_bytes(xs.size, 16000)
        lead, trail, mark = 64, 4096, 0xA5
        buf = torch.full((lead + need + trail,), mark, device=DEV, dtype=torch.uint8)
        assert (buf.data_ptr() + lead) % 8 == 0
        xs_g = torch.from_numpy(xs).to(DEV)
        lk = torch.zeros((), device=DEV)
        cn = torch.zeros(3, device=DEV, dtype=torch.int32)
        rc = lib.knnsvc_loudness(ops._p(xs_g), xs.size, 16000, ops._p(lk), ops._p(cn), ctypes.c_void_p(buf.data_ptr() + lead), need, ops._stream())
        torch.cuda.synchronize()
        clean = bool((buf[:lead] == mark).all()) and bool((buf[lead + need:] == mark).all())
        note(f"oracle/exact-workspace/{nm}", rc == 0 and clean and close_db(float(lk), w0, TOL_DB) and tuple(cn.cpu().tolist()) == c0,
             f"rc {rc}, {need} bytes, sentinels intact {clean}, lkfs {float(lk)!r} / {w0!r}")
        rc = lib.knnsvc_loudness(ops._p(xs_g), xs.size, 16000, ops._p(lk), ops._p(cn), ctypes.c_void_p(buf.data_ptr() + lead), need - 1, ops._stream())
        note(f"oracle/short-workspace-refused/{nm}", rc != 0 and b"workspace" in lib.knnsvc_last_error(), f"rc {rc}")


# ------------------------------------------------------------------ 2. determinism
def case_determinism():
    xg = torch.from_numpy(long_clip()).to(DEV)
    a, ca = ops.loudness(xg, return_counts=True)
    b, cb = ops.loudness(xg, return_counts=True)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        c, cc = ops.loudness(xg, return_counts=True)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    note("determinism/clip30s", same(a, b) and same(a, c) and same(ca, cb) and same(ca, cc),
         f"{float(a)!r} {float(b)!r} {float(c)!r}")


# ------------------------------------------------------------------ 3. gain
def case_gain():
    x = O.gated_signal()
    xg = torch.from_numpy(x).to(DEV)
    for target in (-16.0, -23.0):
        out, lk = ops.normalize_loudness(xg, target)
        g = np.float32(10.0 ** ((target - float(lk)) / 20.0))
        ok_mul = np.allclose(out.cpu().numpy(), x * g, rtol=2e-6, atol=0)
        after = O.loudness(out.cpu().numpy(), 16000)
        note(f"gain/target{target:g}", ok_mul and abs(after - target) <= 3e-4 and same(xg, torch.from_numpy(x).to(DEV)),
             f"lkfs {float(lk)!r}, g {float(g)!r}, out == x g: {ok_mul}, oracle loudness of out {after!r}")
        inplace = xg.clone()
        out2, lk2 = ops.normalize_loudness(inplace, target, out=inplace)
        note(f"gain/in-place/target{target:g}", out2 is inplace and same(inplace, out) and same(lk, lk2), "")
    for name, sil in (("n6399", noise(6399, 1)), ("zeros8000", np.zeros(8000, np.float32))):
        sg = torch.from_numpy(sil).to(DEV)
        out, lk = ops.normalize_loudness(sg, -16.0)
        note(f"gain/no-loudness/{name}", float(lk) == -math.inf and same(out, sg), f"lkfs {float(lk)!r}")


# ------------------------------------------------------------------ 4. product
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
    vc = tiny_vc("mix")
    tv = serving.TargetVoice(vc, pool)
    mk = lambda **kw: serving.BatchConverter(vc, tv, "mix", "post_opt_0.2", **kw)
    off = [y.clone() for y in mk().convert(files)]
    off2 = mk(loudness_db=None).convert(files)
    bad = [i for i in range(len(files)) if not same(off[i], off2[i])]
    note("product/off-twice", not bad, f"sources that differ: {bad}")
    want = [ops.normalize_loudness(y, -20.0)[0] for y in off]
    levels = [float(ops.loudness(y)) for y in off]
    for route, kw in (("lanes", dict(match="lanes")), ("segmented", dict(match="segmented", match_batch=4))):
        on = mk(loudness_db=-20, **kw).convert(files)
        bad = [i for i in range(len(files)) if not same(on[i], want[i])]
        note(f"product/on/{route}", not bad and len(on) == len(files), f"sources that differ: {bad}; levels of the off run {levels}")
    # special_match: one source against one target FILE, against the converter on the same pair
    ref = os.path.join(pool, "t0.wav")
    tv1 = serving.TargetVoice(vc, ref)
    src = files[0]
    y_off = serving.BatchConverter(vc, tv1, "mix", "post_opt_0.2").convert([src])[0]
    y_on = serving.BatchConverter(vc, tv1, "mix", "post_opt_0.2", loudness_db=-20).convert([src])[0]
    out_file = os.path.join(srcd, "s0_to_t0_knn_mix_post_opt_0.2.wav")
    pcm = lambda y: audio_io.to_pcm32(y.detach().cpu().numpy()[None])
    for tag, kw, y in (("on", dict(normalize_loudness=True, tgt_loudness_db=-20), y_on),
                       ("level-none", dict(normalize_loudness=True, tgt_loudness_db=None), y_off),
                       ("switch-off", dict(tgt_loudness_db=-20), y_off)):
        if os.path.isfile(out_file):
            os.remove(out_file)
        vc.special_match(src, ref, ckpt_type="mix", post_opt="post_opt_0.2", **kw)
        x, sr = audio_io.read_wav(out_file)
        note(f"product/special_match/{tag}", sr == 16000 and np.array_equal(audio_io.to_pcm32(x), pcm(y)), "")
    note("product/special_match/on-differs-from-off", not np.array_equal(pcm(y_on), pcm(y_off)), "")
    # bulk_match on two tiny speakers, both directions, default target -16
    root = os.path.join(tmp, "data")
    for s, spk in enumerate(("spkA", "spkB")):
        os.makedirs(os.path.join(root, spk))
        for u in range(2):
            write_clip(os.path.join(root, spk, f"u{u}.wav"), 3 * 16000 + 500 * u + 77 * s, 1000 * s + u + 40, f0_mul=1.25 if s == 0 else 1.0)
    read = lambda p: audio_io.read_wav(p)[0][0].astype(np.float64)
    off_files = vc.bulk_match(root, root, os.path.join(tmp, "bulk_off"), ckpt_type="mix", post_opt="post_opt_0.2")
    # precondition, by the oracle on the off run: -16 stays below full scale for every file (the peak rule of to_pcm32 must not fire)
    would_peak = []
    for p in off_files:
        x = read(p)
        would_peak.append(float(np.abs(x).max()) * 10.0 ** ((-16.0 - O.loudness(x, 16000)) / 20.0))
    note("product/bulk_match/precondition-below-full-scale", len(off_files) == 4 and max(would_peak) < 1.0,
         f"peaks at -16 LKFS predicted from the off run: {would_peak}")
    on_files = vc.bulk_match(root, root, os.path.join(tmp, "bulk_on"), ckpt_type="mix", post_opt="post_opt_0.2", normalize_loudness=True)
    got = [O.loudness(read(p), 16000) for p in on_files]
    excluded = [os.path.basename(p) for p, pk in zip(on_files, would_peak) if pk > 1.0]
    ok = [abs(l + 16.0) <= 1e-3 for l, pk in zip(got, would_peak) if pk <= 1.0]
    note("product/bulk_match/files-at-target", len(on_files) == 4 and all(ok) and not excluded,
         f"loudness of the written files {got}; excluded for the peak rule: {excluded} (cap: none)")
    names = lambda fs, d: sorted(os.path.relpath(p, os.path.join(tmp, d)) for p in fs)
    note("product/bulk_match/same-file-names", names(on_files, "bulk_on") == names(off_files, "bulk_off"), "")


if __name__ == "__main__":
    sys.exit(run_cases([("oracle", case_oracle), ("determinism", case_determinism), ("gain", case_gain), ("product", case_product)], sys.argv[1]))
