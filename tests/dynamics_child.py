"""Child interpreter of tests/test_gpu_dynamics.py: runs every output-dynamics case on the GPU and writes a JSON report
{check name: {"ok": bool, "detail": str}}; the pytest process only reads it (it must not initialise the GPU itself).

    python tests/dynamics_child.py REPORT.json

The reference is tests/dynamics_oracle.py (fp64 numpy).  Tolerances, none of them taken from what the kernels give:
  envelope gains G     1e-9 relative: a sum of N <= 2^20 non-negative terms is off by at most N 2^-53 = 1.2e-10 in any order; sqrt,
                       the divisions and pow add a few ulp; that leaves about a factor 8 of margin
  waveforms            one fp32 ulp: two fp64 products that agree to 1e-9 (the envelope) or to a few 1e-16 (the ceiling) round to
                       the same or to adjacent floats
  ceiling statistics   the count exactly; the smallest gain to 1e-13 relative (fp64 with a few hundred roundings)
  ceiling property     max |out| <= c (1 + 2^-23), on the device output itself
Everything else is bit equality.  The largest observed errors go into the report ("envelope/max-error", "ceiling/max-error")."""
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

import dynamics_oracle as O
from knn_svc_amd import _lib, audio_io, ops
from tests.gpu_child import DEV, dev, misaligned, note, run_cases, same, tiny_vc, write_clip

HOP = 320
TOL_G, TOL_MIN = 1e-9, 1e-13
WORST = {"G": 0.0, "env_ulp": 0, "lim_ulp": 0, "min_gain": 0.0}


def ulps(a, b):
    """Largest distance between two fp32 arrays in units in the last place (0 for empty arrays; huge when a NaN is involved)."""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    if a.shape != b.shape:
        return 1 << 40
    if a.size == 0:
        return 0
    if not (np.isfinite(a).all() and np.isfinite(b).all()):
        return 1 << 40
    key = lambda v: np.where(v.view(np.int32) < 0, -(v.view(np.int32).astype(np.int64) & 0x7FFFFFFF), v.view(np.int32).astype(np.int64))
    return int(np.abs(key(a) - key(b)).max())


# ------------------------------------------------------------------ 1. envelope mix against the oracle
def env_check(name, y, x, a, hop=HOP, got=None):
    want, wG = O.envelope_mix(y, x, a, hop)
    if got is None:
        got = ops.envelope_mix(dev(y), dev(x), a, hop=hop, return_gains=True)
    out, G = got[0].cpu().numpy(), got[1].cpu().numpy()
    eG = float(np.abs(G / wG - 1).max()) if G.shape == wG.shape else float("inf")
    eu = ulps(out, want)
    WORST["G"], WORST["env_ulp"] = max(WORST["G"], eG), max(WORST["env_ulp"], eu)
    note(f"envelope/{name}", eG <= TOL_G and eu <= 1, f"T {len(y) // hop}, hop {hop}, a {a}: G rel err {eG:.2e}, waveform {eu} ulp")
    return got


def case_envelope():
    lib = _lib.load()
    swell = lambda n, seed: (O.noise(n, seed) * (0.3 + np.linspace(0, 1, n) ** 2)).astype(np.float32)
    for T, hop in ((1, HOP), (2, HOP), (3, HOP), (64, HOP), (5, 64)):
        env_check(f"T{T}-hop{hop}", O.sines(T * hop, 10 + T), swell(T * hop, 20 + T), 0.6, hop)
    T = 64
    N = T * HOP
    y, x = O.sines(N, 31), O.phrased(T + 4, 32)
    for tag, nx in (("one-sample-short", N - 1), ("one-block-short", N - HOP), ("half", N // 2), ("longer", N + 517)):
        env_check(f"source-{tag}", y, x[:nx], 0.6)
    for a in (0.25, 0.5, 1.0):
        env_check(f"phrased-a{a}", y, x[:N], a)
    for tag, yy, xx in (("silent-source", y, np.zeros(N, np.float32)), ("silent-output", np.zeros(N, np.float32), x[:N])):
        out, G = env_check(tag, yy, xx, 0.7)
        note(f"envelope/{tag}-is-y-bit-for-bit", same(out, dev(yy)) and bool((G == 1).all()), "")
    out, G = ops.envelope_mix(dev(y), torch.zeros(0, device=DEV), 0.7, return_gains=True)
    note("envelope/empty-source-is-y-bit-for-bit", same(out, dev(y)) and bool((G == 1).all()), "")
    # level invariance: the same source 40 dB lower, the scaling exact in fp32 (multiples of 2^-20 below 2^-3, times 100)
    m = np.round(x[:N].astype(np.float64) * 0.1 * 2 ** 20)
    lo, hi = (m / 2 ** 20).astype(np.float32), (100 * m / 2 ** 20).astype(np.float32)
    g_hi = env_check("level/equal", y, hi, 0.5)
    g_lo = env_check("level/40dB-below", y, lo, 0.5)
    eG = float((g_lo[1] / g_hi[1] - 1).abs().max())
    eu = ulps(g_lo[0].cpu().numpy(), g_hi[0].cpu().numpy())
    note("envelope/level/invariant", eG <= TOL_G and eu <= 1,
         f"source rms {float(np.sqrt((lo.astype(np.float64) ** 2).mean())):.4f} against {float(np.sqrt((hi.astype(np.float64) ** 2).mean())):.4f}: "
         f"G rel diff {eG:.2e}, waveform {eu} ulp")
    # in place, gains = NULL, misaligned pointers: the same bits as the plain call
    ref_out, ref_G = ops.envelope_mix(dev(y), dev(x[:N]), 0.5, return_gains=True)
    buf = dev(y)
    r = ops.envelope_mix(buf, dev(x[:N]), 0.5, out=buf, return_gains=True)
    note("envelope/in-place", r[0] is buf and same(buf, ref_out) and same(r[1], ref_G), "")
    note("envelope/gains-null", same(ops.envelope_mix(dev(y), dev(x[:N]), 0.5), ref_out), "")
    ym, xm, om = misaligned(y), misaligned(x[:N]), misaligned(np.zeros(N, np.float32))
    r = ops.envelope_mix(ym, xm, 0.5, out=om, return_gains=True)
    note("envelope/pointers-4-bytes-off-alignment", same(om, ref_out) and same(r[1], ref_G), f"y % 16 = {ym.data_ptr() % 16}, out % 16 = {om.data_ptr() % 16}")
    # a workspace of exactly the reported size between sentinel bytes
    need = lib.knnsvc_envelope_workspace_bytes(N, HOP)
    lead, trail, mark = 64, 4096, 0xA5
    ws = torch.full((lead + need + trail,), mark, device=DEV, dtype=torch.uint8)
    assert (ws.data_ptr() + lead) % 8 == 0
    yg, xg, og, Gg = dev(y), dev(x[:N]), torch.zeros(N, device=DEV), torch.zeros(T, device=DEV, dtype=torch.float64)
    call = lambda n, hop, nbytes: lib.knnsvc_envelope_mix(ops._p(yg), n, ops._p(xg), N, hop, 0.5, ops._p(og), ops._p(Gg),
                                                          ctypes.c_void_p(ws.data_ptr() + lead), nbytes, ops._stream())
    rc = call(N, HOP, need)
    torch.cuda.synchronize()
    clean = bool((ws[:lead] == mark).all()) and bool((ws[lead + need:] == mark).all())
    note("envelope/exact-workspace", rc == 0 and clean and same(og, ref_out) and same(Gg, ref_G), f"rc {rc}, {need} bytes, sentinels intact {clean}")
    rc = call(N, HOP, need - 1)
    note("envelope/short-workspace-refused", rc != 0 and b"workspace" in lib.knnsvc_last_error(), f"rc {rc}")
    # error codes, nothing launched: the output buffer keeps its marker
    og.fill_(7.0)
    rc1, rc2 = call(N - 1, HOP, need), call(N - N % 100, 100, need)
    z1, z2 = lib.knnsvc_envelope_workspace_bytes(N - 1, HOP), lib.knnsvc_envelope_workspace_bytes(N - N % 100, 100)
    torch.cuda.synchronize()
    note("envelope/bad-length-and-bad-hop-are-error-codes", rc1 != 0 and rc2 != 0 and z1 == 0 and z2 == 0 and bool((og == 7.0).all()),
         f"rc {rc1}, {rc2}; workspace_bytes {z1}, {z2}")
    note("envelope/max-error", True, f"largest over all cases: G rel err {WORST['G']:.3e} (bound {TOL_G:g}), waveform {WORST['env_ulp']} ulp (bound 1)")


# ------------------------------------------------------------------ 2. peak ceiling against the oracle
P6 = 20 * math.log10(0.5)


def lim_check(name, y, p=P6, sr=16000, got=None):
    y = np.ascontiguousarray(y, dtype=np.float32)
    want, wcount, wmin = O.limit_peak(y, p, sr)
    if got is None:
        got = ops.limit_peak(dev(y), p, sr, return_stats=True)
    out, count, smin = got[0].cpu().numpy(), int(got[1][0]), float(got[1][1])
    c = 10.0 ** (p / 20.0)
    eu, emin = ulps(out, want), abs(smin / wmin - 1)
    under = float(np.abs(out.astype(np.float64)).max()) <= c * (1 + 2.0 ** -23) if out.size else True
    WORST["lim_ulp"], WORST["min_gain"] = max(WORST["lim_ulp"], eu), max(WORST["min_gain"], emin)
    note(f"ceiling/{name}", eu <= 1 and count == wcount and emin <= TOL_MIN and under,
         f"n {y.size}, sr {sr}, p {p:.3f}: waveform {eu} ulp, count {count} / {wcount}, min gain {smin!r} / {wmin!r}, under the ceiling {under}")
    return got, (wcount, wmin)


def case_ceiling():
    lib = _lib.load()
    tile, L = ops.peak_limit_layout()
    assert L == O.lookahead(16000)
    for tag, n in (("0", 0), ("1", 1), ("L", L), ("L+1", L + 1), ("2L", 2 * L), ("2L+1", 2 * L + 1), ("4L+1", 4 * L + 1), ("tile-1", tile - 1),
                   ("tile", tile), ("tile+1", tile + 1), ("3tile+L+1", 3 * tile + L + 1)):
        lim_check(f"length/{tag}", O.noise(n, 300 + n % 97, amp=0.8))
    n = 3 * tile + L + 1
    quiet = np.clip(O.noise(n, 41), -0.4, 0.4)

    def peaks(*at, v=0.9):
        y = quiet.copy()
        y[list(at)] = v
        return y
    for tag, at in (("0", 0), ("n-1", n - 1), ("tile-1", tile - 1), ("tile", tile), ("tile-2L", tile - 2 * L), ("tile+2L", tile + 2 * L)):
        _, (wcount, wmin) = lim_check(f"peak-at/{tag}", peaks(at))
        lo, hi = max(0, at - 2 * L), min(n - 1, at + 2 * L)
        note(f"ceiling/peak-at/{tag}-oracle-precondition", wcount == hi - lo + 1 and abs(wmin / (0.5 / np.float64(np.float32(0.9))) - 1) < 1e-14,
             f"the oracle touches {wcount} samples, min gain {wmin!r}")
    lim_check("two-peaks/2L-apart", peaks(tile + 100, tile + 100 + 2 * L))
    lim_check("two-peaks/2L+1-apart", peaks(tile + 100, tile + 100 + 2 * L + 1))
    lim_check("negative-peak", peaks(tile + 7, v=-0.9))
    plateau = quiet.copy()
    plateau[tile - 300:tile + 500] = 0.9
    lim_check("plateau-across-a-tile-boundary", plateau)
    lim_check("everything-over", np.full(n, 0.9, np.float32))
    lim_check("44100-Hz", O.noise(tile + 1000, 43, amp=0.8), sr=44100)
    lim_check("44100-Hz-peak-at-tile-2L", peaks(tile - 2 * O.lookahead(44100)), sr=44100)
    loud = O.noise(n, 44, amp=1.5)
    for p in (0.0, -1.0, -6.0):
        lim_check(f"p{p:g}", loud, p=p)
    # identity: a signal under the ceiling comes back bit-identical, with empty statistics
    out, (count, smin) = ops.limit_peak(dev(quiet), P6, return_stats=True)
    note("ceiling/identity", same(out, dev(quiet)) and int(count) == 0 and float(smin) == 1.0, f"count {int(count)}, min gain {float(smin)!r}")
    # in place, misaligned, stats = NULL: the same bits as the plain call
    y = peaks(5, tile - 1, tile + 2 * L, 2 * tile + 9, n - 3)
    y[tile + 900:tile + 1400] *= 2.5
    (ref, rstats), _ = lim_check("several", y)
    buf = dev(y)
    r = ops.limit_peak(buf, P6, out=buf, return_stats=True)
    note("ceiling/in-place", r[0] is buf and same(buf, ref) and same(r[1][0], rstats[0]) and same(r[1][1], rstats[1]), "")
    ym, om = misaligned(y), misaligned(np.zeros(n, np.float32))
    r = ops.limit_peak(ym, P6, out=om, return_stats=True)
    note("ceiling/pointers-4-bytes-off-alignment", same(om, ref) and same(r[1][0], rstats[0]), f"y % 16 = {ym.data_ptr() % 16}")
    note("ceiling/stats-null", same(ops.limit_peak(dev(y), P6), ref), "")
    yg, og = dev(y), torch.full((n,), 7.0, device=DEV)
    call = lambda sr, p: lib.knnsvc_peak_limit(ops._p(yg), n, sr, p, ops._p(og), None, ops._stream())
    rcs = [call(4000, -6.0), call(16000, 1.0), call(16000, float("nan")), call(16000, float("-inf"))]
    torch.cuda.synchronize()
    note("ceiling/bad-rate-and-bad-level-are-error-codes", all(rc != 0 for rc in rcs) and bool((og == 7.0).all()), f"rc {rcs}")
    note("ceiling/max-error", True, f"largest over all cases: waveform {WORST['lim_ulp']} ulp (bound 1), min gain rel err {WORST['min_gain']:.3e} (bound {TOL_MIN:g})")


# ------------------------------------------------------------------ 3. determinism
def case_determinism():
    n = 480000
    t = np.arange(n) / 16000.0
    y = ((0.3 + 0.6 * np.sin(2 * np.pi * 0.21 * t) ** 2) * np.sin(2 * np.pi * (150.0 * t + 7.5 * t * t))).astype(np.float32) + O.noise(n, 51, 0.01)
    yg, xg = dev(y), dev(O.phrased(n // HOP, 52))

    def both():
        e, G = ops.envelope_mix(yg, xg, 0.7, return_gains=True)
        o, st = ops.limit_peak(e, -6.0, return_stats=True)
        return e, G, o, st[0], st[1]
    a, b = both(), both()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        c = both()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    note("determinism/clip30s", all(same(u, v) and same(u, w) for u, v, w in zip(a, b, c)) and int(a[3]) > 0,
         f"limited samples {int(a[3])}, smallest gain {float(a[4])!r}")


# ------------------------------------------------------------------ 4. product
def phrase_gain(n, seed):
    """A phrased envelope for a clip: stretches of 0.2 .. 0.5 s, alternately at a level of their own (0.15 .. 1) and silent."""
    rng = np.random.default_rng(seed)
    g = np.zeros(n)
    i, on = 0, True
    while i < n:
        ln = int(rng.uniform(0.2, 0.5) * 16000)
        if on:
            g[i:i + ln] = rng.uniform(0.15, 1.0)
        i, on = i + ln, not on
    return g


def case_product(tmp):
    from knn_svc_amd import matching as M, serving
    pool = os.path.join(tmp, "tgt"); os.makedirs(pool)
    for i in range(4):
        write_clip(os.path.join(pool, f"t{i}.wav"), 3 * 16000 + 37 * i, 900 + i)
    srcd = os.path.join(tmp, "src"); os.makedirs(srcd)
    lens = [16000 * 2 + 11, 16000 * 3, 9000, 16000 * 2 + 11, 16000 + 641, 40000]
    files = []
    for i, n in enumerate(lens):
        files.append(os.path.join(srcd, f"s{i}.wav"))
        write_clip(files[-1], n, 700 + i, f0_mul=1.2, gain=phrase_gain(n, 700 + i + 5000))
    srcs = [dev(M.load_utterance(f)[0]) for f in files]
    vc = tiny_vc("mix")
    tv = serving.TargetVoice(vc, pool)
    mk = lambda **kw: serving.BatchConverter(vc, tv, "mix", "post_opt_0.2", **kw)
    differ = lambda got, want: [i for i in range(len(want)) if not same(got[i], want[i])]
    off = [y.clone() for y in mk().convert(files)]
    off2 = mk(envelope_mix=None, peak_db=None).convert(files)
    note("product/off-twice", not differ(off2, off), f"sources that differ: {differ(off2, off)}")
    db = lambda ys: min(0.0, 20 * math.log10(0.5 * max(float(y.abs().max()) for y in ys)))
    # envelope mix, then the ceiling at half the off run's largest peak
    q = db(off)
    mixed = [ops.envelope_mix(y, s, 0.7) for y, s in zip(off, srcs)]
    want, engaged = [], 0
    for m in mixed:
        o, st = ops.limit_peak(m, q, return_stats=True)
        want.append(o); engaged += int(st[0])
    note("product/on/precondition", engaged > 0 and all(not same(m, y) for m, y in zip(mixed, off)),
         f"q {q:.2f} dBFS, limited samples {engaged}, off-run peaks {[round(float(y.abs().max()), 4) for y in off]}")
    routes = (("lanes", dict(match="lanes")), ("segmented", dict(match="segmented", match_batch=4)))
    for route, kw in routes:
        on = mk(envelope_mix=0.7, peak_db=q, **kw).convert(files)
        note(f"product/on/{route}", not differ(on, want) and len(on) == len(files), f"sources that differ: {differ(on, want)}")
    # with loudness: mix, then loudness, then the ceiling
    levelled = [ops.normalize_loudness(m, -20.0)[0] for m in mixed]
    q2 = db(levelled)
    want2 = [ops.limit_peak(v, q2) for v in levelled]
    for route, kw in routes:
        on = mk(envelope_mix=0.7, peak_db=q2, loudness_db=-20, **kw).convert(files)
        note(f"product/order/{route}", not differ(on, want2) and any(not same(a, b) for a, b in zip(want2, levelled)),
             f"q {q2:.2f} dBFS; sources that differ: {differ(on, want2)}")
    # a RequestQueue in front of such a converter
    rq = serving.RequestQueue(mk(envelope_mix=0.7, peak_db=q), max_batch=8, max_wait_ms=200.0)
    try:
        got = [f.result(timeout=120).to(DEV) for f in [rq.submit(p) for p in files]]
    finally:
        rq.close()
    note("product/request-queue", not differ(got, want), f"batches {rq.batches}; sources that differ: {differ(got, want)}")
    # special_match: one source against one target FILE, against the converter on the same pair
    ref = os.path.join(pool, "t0.wav")
    tv1 = serving.TargetVoice(vc, ref)
    src = files[0]
    one = lambda **kw: serving.BatchConverter(vc, tv1, "mix", "post_opt_0.2", **kw).convert([src])[0]
    y_off = one()
    q1 = db([y_off])
    c1 = 10.0 ** (q1 / 20.0)
    y_on = one(envelope_mix=0.7, peak_db=q1)
    out_file = os.path.join(srcd, "s0_to_t0_knn_mix_post_opt_0.2.wav")
    pcm = lambda y: audio_io.to_pcm32(y.detach().cpu().numpy()[None])

    def written(**kw):
        if os.path.isfile(out_file):
            os.remove(out_file)
        vc.special_match(src, ref, ckpt_type="mix", post_opt="post_opt_0.2", **kw)
        x, sr = audio_io.read_wav(out_file)
        assert sr == 16000
        return x
    x = written(envelope_mix=0.7, peak_db=q1)
    note("product/special_match/on", np.array_equal(audio_io.to_pcm32(x), pcm(y_on)) and float(np.abs(x).max()) <= c1 * (1 + 2.0 ** -23),
         f"file peak {float(np.abs(x).max())!r}, ceiling {c1!r}")
    note("product/special_match/defaults", np.array_equal(audio_io.to_pcm32(written()), pcm(y_off)), "")
    note("product/special_match/on-differs-from-off", not np.array_equal(pcm(y_on), pcm(y_off)), "")
    # the gap the loudness docstring names: normalised past full scale, the file used to be divided by its peak
    target = float(ops.loudness(y_off)) + 20 * math.log10(2.0 / float(y_off.abs().max()))           # puts the peak at 2.0
    hot = ops.normalize_loudness(y_off, target)[0]
    capped = ops.limit_peak(hot, -1.0)
    x = written(normalize_loudness=True, tgt_loudness_db=target, peak_db=-1.0)
    c = 10.0 ** (-1.0 / 20.0)
    note("product/special_match/no-peak-division", float(hot.abs().max()) > 1.5 and float(np.abs(x).max()) <= c * (1 + 2.0 ** -23)
         and float(capped.abs().max()) <= 1.0 and np.array_equal(audio_io.to_pcm32(x), pcm(capped)),       # (to_pcm32 divides only above 1)
         f"peak before the ceiling {float(hot.abs().max()):.3f}, file peak {float(np.abs(x).max())!r}, ceiling {c!r}")
    # bulk_match on two tiny speakers, both directions
    root = os.path.join(tmp, "data")
    for s, spk in enumerate(("spkA", "spkB")):
        os.makedirs(os.path.join(root, spk))
        for u in range(2):
            n, seed = 3 * 16000 + 500 * u + 77 * s, 1000 * s + u + 40
            write_clip(os.path.join(root, spk, f"u{u}.wav"), n, seed, f0_mul=1.25 if s == 0 else 1.0, gain=phrase_gain(n, seed + 5000))
    read = lambda p: audio_io.read_wav(p)[0][0].astype(np.float64)
    off_files = vc.bulk_match(root, root, os.path.join(tmp, "bulk_off"), ckpt_type="mix", post_opt="post_opt_0.2")
    off_peaks = [float(np.abs(read(p)).max()) for p in off_files]
    qb = min(0.0, 20 * math.log10(0.5 * min(off_peaks)))             # under every file's own peak: every file is limited
    cb = 10.0 ** (qb / 20.0)
    on_files = vc.bulk_match(root, root, os.path.join(tmp, "bulk_on"), ckpt_type="mix", post_opt="post_opt_0.2", peak_db=qb)
    on_peaks = [float(np.abs(read(p)).max()) for p in on_files]
    note("product/bulk_match/files-under-the-ceiling", len(on_files) == 4 and all(cb * 0.5 < pk <= cb * (1 + 2.0 ** -23) for pk in on_peaks),
         f"ceiling {cb!r}; peaks off {off_peaks}, on {on_peaks}")
    mix_files = vc.bulk_match(root, root, os.path.join(tmp, "bulk_mix"), ckpt_type="mix", post_opt="post_opt_0.2", envelope_mix=0.7, peak_db=qb)
    mix_peaks = [float(np.abs(read(p)).max()) for p in mix_files]
    changed = [not np.array_equal(read(a), read(b)) for a, b in zip(mix_files, on_files)]
    note("product/bulk_match/with-the-envelope-mix", len(mix_files) == 4 and all(pk <= cb * (1 + 2.0 ** -23) for pk in mix_peaks) and all(changed),
         f"peaks {mix_peaks}")
    names = lambda fs, d: sorted(os.path.relpath(p, os.path.join(tmp, d)) for p in fs)
    note("product/bulk_match/same-file-names", names(on_files, "bulk_on") == names(off_files, "bulk_off") == names(mix_files, "bulk_mix"), "")


if __name__ == "__main__":
    sys.exit(run_cases([("envelope", case_envelope), ("ceiling", case_ceiling), ("determinism", case_determinism), ("product", case_product)],
                       sys.argv[1]))
