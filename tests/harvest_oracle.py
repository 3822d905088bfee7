"""Harvest f0 (csrc/harvest.hip) stage by stage: the seeded cases, the staged references and the margin rules that
tests/harvest_child.py (GPU) and tests/test_harvest_cpu.py (no GPU) share.  Plain numpy; importing it touches neither the GPU
nor knn_svc_amd.

Every staged reference takes the INPUTS of its stage as arrays and returns what oracle/f0_ref.py computes from them, by calling
that file's functions.  The child feeds stage s with the device's own output of stage s - 1 (teacher forcing), so that a last-bit
difference in the band-pass bank cannot cascade into another contour and hide what the later stages do; ``chain`` feeds each
stage with the previous reference instead and so restates f0_ref.harvest, bit for bit.

Decision stages make hard decisions on fp64 values that the two sides compute with the same few operations; they can differ
by contraction and by the order of short sums only.  A gate whose margin in the ORACLE is below MARGIN (relative to its
threshold) is excluded: the element takes the device's value before anything after it is compared, and the exclusions are
counted against CAP of the stage's elements.  The decisions that steer everything after them (hlen, the kept sections, every
selection of the extension, the merge order and every merge step) allow no exclusion at all: ``steering_margins`` must be clean."""
import math

import numpy as np

from oracle import f0_ref

FS = 16000
MARGIN = 1e-9                 # relative distance of a gate's operand from its threshold below which the gate is not compared
CAP = 1e-3                    # share of a stage's elements that may be excluded per case
VALUE_TOL = 2.0 ** -40        # decision stages: values, relative to the larger operand
NC, NS = 16, 112              # candidate slots per frame before / after the overlap (HV_NC, HV_NS)
DEFAULT = (65.0, 1047.0, 20.0, 80.0)          # f0_floor, f0_ceil, frame_period, zero_below

# the arrays of the workspace in the order knnsvc_debug_f0_harvest_layout writes them, with their element types
ARRAYS = (("t1", "f8"), ("t2", "f8"), ("mean", "f8"), ("ypad", "f8"), ("bf0", "f8"), ("hlen", "i4"), ("filt", "f8"), ("events", "f8"),
          ("ecount", "i4"), ("raw", "f8"), ("cand0", "f8"), ("cand", "f8"), ("score", "f8"), ("cand2", "f8"), ("score2", "f8"),
          ("base", "f8"), ("s1", "f8"), ("s2", "f8"), ("s3", "f8"), ("s4", "f8"), ("sm", "f8"), ("st", "i4"), ("ed", "i4"),
          ("xst", "i4"), ("xed", "i4"), ("keep", "i4"), ("order", "i4"), ("gst", "i4"), ("ged", "i4"), ("woff", "i8"), ("soff", "i8"),
          ("chan", "f8"), ("chs", "f8"), ("ms", "f8"), ("scratch", "f8"), ("info", "i4"))
DIMS = ("total", "nch", "ylen", "ld", "nfr", "nout", "ecap", "scap", "chan_cap", "scratch_cap", "HV_NC", "HV_NS", "HV_YPAD", "HV_MARG",
        "HV_SMOOTH_MARG")
N_TABLE = 2 * len(ARRAYS) + len(DIMS)


def parse_layout(table):
    """The layout entry's table -> ({array: (offset, bytes)}, {dimension: value})."""
    t = [int(v) for v in table]
    arr = {name: (t[2 * i], t[2 * i + 1]) for i, (name, _) in enumerate(ARRAYS)}
    return arr, dict(zip(DIMS, t[2 * len(ARRAYS):]))


# ------------------------------------------------------------------ cases
def _tone(n, f, harmonics=4, seed=0, noise=1e-3, amp=0.3):
    t = np.arange(n) / FS
    x = sum(np.sin(2 * np.pi * k * f * t + 0.3 * k) / k for k in range(1, harmonics + 1)) * amp
    return x + noise * np.random.default_rng(seed).standard_normal(n)


def _bursts(n, f, on_ms, off_ms, seed, every_second=1.0, noise=0.0, skip=0):
    """Bursts of a three-harmonic tone with digital silence between them; every skip-th burst is left out."""
    t = np.arange(n) / FS
    x = np.zeros(n)
    on, off = on_ms * FS // 1000, off_ms * FS // 1000
    for b, s in enumerate(range(off, n - on, on + off)):
        if skip and b % skip == skip - 1:
            continue
        fb = f * (every_second if b % 2 else 1.0)
        tt = t[s:s + on] - t[s]
        x[s:s + on] = 0.3 * sum(np.sin(2 * np.pi * k * fb * tt) / k for k in range(1, 4)) * np.hanning(on + 2)[1:-1] ** 0.25
    return x + noise * np.random.default_rng(seed).standard_normal(n)


def _natural():
    from knn_svc_amd import synthetic
    return synthetic.synth_clip(24077, 3)[0]


def _two_voices():
    return _tone(24000, 130.0, 4, 21) * 0.6 + _tone(24000, 207.0, 4, 22) * 0.6


def _weak():
    t = np.arange(16000) / FS
    return 0.02 * sum(np.sin(2 * np.pi * k * 68.0 * t) / k for k in range(1, 4)) + 0.1 * np.random.default_rng(1).standard_normal(16000)


GENERATORS = {
    "min": (1600, lambda: _tone(1600, 220.0, 4, 1)),
    "tile-1024": (2048, lambda: _tone(2048, 440.0, 3, 2)),
    "tile-1025": (2049, lambda: _tone(2049, 440.0, 3, 3)),
    "chunk-4078": (4078, lambda: _tone(4078, 330.0, 3, 4)),
    "chunk-4079": (4079, lambda: _tone(4079, 330.0, 3, 5)),
    "natural": (24077, _natural),
    # the 20 ms gaps are bridged (under 9 frames are left of them), so every sixth burst is left out: several final sections
    "dense": (24000, lambda: _bursts(24000, 400.0, 12, 20, 6, skip=6)),
    "merge": (24000, lambda: _bursts(24000, 180.0, 40, 10, 7, every_second=1.3)),
    "two-voices": (24000, _two_voices),
    "noise": (16000, lambda: 0.1 * np.random.default_rng(8).standard_normal(16000)),
    "silence": (16000, lambda: np.zeros(16000)),
    "low-70": (24000, lambda: _tone(24000, 70.0, 10, 9)),
    "dc": (16000, lambda: _tone(16000, 220.0, 4, 1) + 0.5),
    # a 68 Hz tone 14 dB under white noise: detection flickers, and a section stays shorter than 2200 / 68 = 32 frames after its
    # extension (two-voices, where such sections were expected, keeps all of its sections)
    "weak": (16000, _weak),
}
# case -> (generator, (f0_floor, f0_ceil, frame_period, zero_below))
CASES = {name: (name, DEFAULT) for name in GENERATORS}
CASES["low-70-zero-0"] = ("low-70", (65.0, 1047.0, 20.0, 0.0))
CASES["params/80-1600-5"] = ("two-voices", (80.0, 1600.0, 5.0, 80.0))
CASES["params/100-500-1"] = ("two-voices", (100.0, 500.0, 1.0, 80.0))
CASES["params/65-1047-12.5"] = ("two-voices", (65.0, 1047.0, 12.5, 80.0))
CASES["params/65-1600-20"] = ("two-voices", (65.0, 1600.0, 20.0, 80.0))          # the most channels the default floor gives: 197
WORKSPACE_CASES = ("natural", "dense", "merge")


def wave(case):
    """-> the case's waveform as the device gets it (float32) and its parameters."""
    gen, params = CASES[case]
    n, fn = GENERATORS[gen]
    x = np.ascontiguousarray(fn(), dtype=np.float32)
    assert x.shape == (n,)
    return x, params


# ------------------------------------------------------------------ dimensions
def dims(L, f0_floor, f0_ceil, frame_period):
    nch = 1 + int(np.log2((f0_ceil * 1.1) / (f0_floor * 0.9)) * 40)
    return {"nch": nch, "ylen": (L - 1) // 2 + 1, "nfr": int(1000.0 * L / FS / 1.0) + 1, "nout": int(1000.0 * L / FS / frame_period) + 1}


def smallest_floor():
    """The smallest float32 f0_floor whose longest band-pass filter fits the bank kernel's tile (half length <= 270 taps and
    within the 288 zeros of padding) and whose longest refinement window fits 384 samples — what hv_check states."""
    def fits(f):
        f = float(np.float32(f))
        b0 = f * 0.9 * 2.0 ** (1.0 / 40.0)
        return int(8000.0 / b0 * 2.0 + 0.5) <= 270 and int(8000.0 / b0 * 2.0 + 0.5) + 1 <= 288 and 2 * int(1.5 * 8000.0 / f + 1.0) + 1 <= 384
    lo, hi = np.float32(60.0), np.float32(70.0)
    assert not fits(lo) and fits(hi)
    while np.nextafter(lo, hi) < hi:
        mid = np.float32((float(lo) + float(hi)) / 2)
        lo, hi = (lo, mid) if fits(mid) else (mid, hi)
    return hi


# ------------------------------------------------------------------ staged references
def ref_decimate(x32):
    return f0_ref.decimate2(np.asarray(x32, np.float64))


def ref_mean(dec):
    """-> (mean by exact summation, the bound on a plain fp64 summation's error: ylen * 2^-53 * max |y|)."""
    return math.fsum(dec) / len(dec), len(dec) * 2.0 ** -53 * float(np.abs(dec).max())


def ref_channels(f0_floor, nch):
    return f0_floor * 0.9 * 2.0 ** ((np.arange(nch) + 1) / 40.0)


def ref_hlen(bf0):
    v = (FS / 2) / bf0 * 2.0
    return f0_ref._round(v).astype(np.int64), np.abs(v - np.floor(v) - 0.5) / v          # margin of the rounding, relative


def ref_bank(y, bf0):
    """y (centred, fp64) and the channel frequencies -> [nch, ylen], through the FFT as the oracle does."""
    afs = FS / 2
    fft_size = int(2 ** (int(np.log(len(y) + 5 + 2 * int(2.0 * afs / bf0[0])) / np.log(2.0)) + 1))
    y_spec = np.fft.rfft(y, fft_size)
    return np.stack([f0_ref._bank_filter(y, y_spec, fft_size, afs, b) for b in bf0])


def ref_events(filt):
    """[nch, ylen] -> per channel the four event lists."""
    return [f0_ref._event_sets(f) for f in filt]


def ref_raw(events, bf0, f0_floor, f0_ceil, nfr):
    """-> (raw [nch, nfr], excluded [nch, nfr]: a gate within MARGIN of its threshold)."""
    afs, tpos = FS / 2, np.arange(nfr) / 1000.0
    raw = np.stack([f0_ref._raw_from_events(e, afs, b, f0_floor, f0_ceil, tpos) for e, b in zip(events, bf0)])
    ung = np.stack([_raw_ungated(e, afs, tpos) for e in events])
    thr = np.stack([np.broadcast_to(np.array([b * 1.1, b * 0.9, f0_ceil, f0_floor])[:, None], (4, nfr)) for b in bf0])      # [nch, 4, nfr]
    near = (np.abs(ung[:, None] - thr) < MARGIN * thr).any(1)
    return raw, near


def _raw_ungated(events, afs, tpos):
    sets = [f0_ref._intervals(e, afs) for e in events]
    if any(s is None or len(s[0]) < 3 for s in sets):
        return np.full(len(tpos), np.inf)
    return np.mean([f0_ref._interp1_extrap(s[0], s[1], tpos) for s in sets], 0)


def ref_detect(raw):
    c = f0_ref._detect_candidates(raw)
    assert c.shape[1] <= NC
    out = np.zeros((raw.shape[1], NC))
    out[:, :c.shape[1]] = c
    return out


def ref_refine(y, cand0, f0_floor, f0_ceil):
    """-> refined f0 and score [nfr, NS], the ungated f0 and deviation, excluded [nfr, NS]."""
    afs, tpos = FS / 2, np.arange(len(cand0)) / 1000.0
    ov = f0_ref._overlap(cand0)
    rf, score = f0_ref._refine(y, afs, tpos, ov, f0_floor, f0_ceil)
    urf, dev = f0_ref._refine_raw(y, afs, tpos, ov)
    on = ov > 0
    with np.errstate(divide="ignore"):
        usc = np.where(on, 1.0 / (1e-12 + dev), 0.0)
    near = on & ((np.abs(urf - f0_floor) < MARGIN * f0_floor) | (np.abs(urf - f0_ceil) < MARGIN * f0_ceil) | (np.abs(usc - 2.5) < MARGIN * 2.5))
    return rf, score, urf, dev, near


def ref_reliable(cand, score):
    """-> (cand2, score2, excluded): a candidate stays when the nearest candidate of a neighbouring frame is within 5 %."""
    c2, s2 = f0_ref._remove_unreliable(cand.copy(), score.copy())
    near = np.zeros(cand.shape, bool)
    for j in range(cand.shape[1]):
        ref = cand[1:-1, j]
        e = np.minimum(f0_ref._select_best(ref, cand[2:], 1.0)[1], f0_ref._select_best(ref, cand[:-2], 1.0)[1])
        near[1:-1, j] = (ref != 0) & (np.abs(e - 0.05) < MARGIN * 0.05)
    return c2, s2, near


def ref_base(cand2, score2):
    return f0_ref._contour_base(cand2, score2)[0]


def ref_step1(base):
    """base -> (s1, excluded): _contour_base picks base from a one-hot candidate table holding it."""
    got, s1 = f0_ref._contour_base(base[:, None].copy(), (base[:, None] > 0).astype(np.float64))
    assert np.array_equal(got, base)
    near = np.zeros(len(base), bool)
    with np.errstate(divide="ignore", invalid="ignore"):
        ref = base[1:-1] * 2 - base[:-2]
        a = np.abs((base[2:] - ref) / ref); b = np.abs(base[2:] - base[1:-1]) / base[1:-1]
        near[2:] = (base[2:] != 0) & ((np.abs(a - 0.008) < MARGIN * 0.008) | (np.abs(b - 0.008) < MARGIN * 0.008))
    return s1, near


def ref_step2(s1):
    s2 = f0_ref._drop_short(s1)
    return s2, f0_ref._boundaries(s2)


def ref_extend(s2, secs, cand2, score2):
    """-> per section (xst, xed, channel [nfr], keep, channel scores [nfr]) and the steering margins of the stage: the smallest
    relative distance of any selection's candidates from the 18 % limit, of the best from the second-best candidate, and of
    2200 / mean from the section length."""
    out, marg = [], []
    for st, ed in secs:
        log = []
        st2, ed2, ch, m, keep = f0_ref._extend_section(s2, st, ed, cand2, 0.18, log)
        cs = np.array([f0_ref._search_score(ch[j], cand2[j], score2[j]) if ch[j] != 0 else 0.0 for j in range(len(ch))])
        out.append((int(st2), int(ed2), ch, keep, cs))
        for p, ref in log:
            t = np.abs(ref - cand2[p]) / ref
            marg.append(float(np.abs(t - 0.18).min() / 0.18))
            u = np.unique(t[t <= 0.18])
            if len(u) > 1:
                marg.append(float((u[1] - u[0]) / 0.18))
        if m > 0:
            marg.append(abs(2200.0 / m - (ed2 - st2)) / (ed2 - st2))
    return out, marg


def ref_merge(ext, s2, cand2, score2):
    """ext as ref_extend returns it -> (kept section ids, order, s3, ms, trace)."""
    kept = [k for k, e in enumerate(ext) if e[3]]
    trace = {"order": [], "steps": []}
    if kept:
        s3 = f0_ref._merge([(ext[k][0], ext[k][1], ext[k][2]) for k in kept], cand2, score2, trace)
    else:
        s3 = s2.copy()
    ms = np.array([f0_ref._search_score(s3[j], cand2[j], score2[j]) if s3[j] != 0 else 0.0 for j in range(len(s3))])
    return kept, trace["order"], s3, ms, trace


def merge_margins(trace):
    """Every score-sum comparison is either equal term by term or apart by more than MARGIN -> the offending steps."""
    return [s for s in trace["steps"] if s["branch"] == "sum" and not s["same_terms"]
            and abs(s["sc1"] - s["sc2"]) <= MARGIN * max(abs(s["sc1"]), abs(s["sc2"]))]


def ref_bridge(s3):
    """-> (s4, the sections the smoother works on, inclusive)."""
    s4 = f0_ref._bridge(s3)
    pad = np.concatenate([[0.0], s4, [0.0]])
    return s4, [(a - 1, b - 1) for a, b in f0_ref._boundaries(pad)]


def ref_smooth(s4):
    return f0_ref._smooth(s4)


def ref_sample(sm, nout, frame_period, zero_below):
    idx = np.minimum(len(sm) - 1, f0_ref._round(np.arange(nout) * frame_period / 1000.0 * 1000.0))
    out = sm[idx].copy()
    out[out < float(np.float32(zero_below))] = 0.0
    return out.astype(np.float32)


# ------------------------------------------------------------------ the whole chain, oracle only
def chain(x32, params):
    """Every staged reference fed with the previous one -> a dict of all intermediates; ``out`` restates f0_ref.harvest."""
    f0_floor, f0_ceil, frame_period, zero_below = params
    d = dims(len(x32), f0_floor, f0_ceil, frame_period)
    r = dict(d)
    r["dec"] = ref_decimate(x32)
    r["y"] = r["dec"] - r["dec"].mean()
    r["bf0"] = ref_channels(f0_floor, d["nch"])
    r["hlen"], r["hlen_margin"] = ref_hlen(r["bf0"])
    r["filt"] = ref_bank(r["y"], r["bf0"])
    r["events"] = ref_events(r["filt"])
    r["raw"], r["raw_near"] = ref_raw(r["events"], r["bf0"], f0_floor, f0_ceil, d["nfr"])
    r["cand0"] = ref_detect(r["raw"])
    r["cand"], r["score"], r["urf"], r["dev"], r["refine_near"] = ref_refine(r["y"], r["cand0"], f0_floor, f0_ceil)
    r["cand2"], r["score2"], r["reliable_near"] = ref_reliable(r["cand"], r["score"])
    r["base"] = ref_base(r["cand2"], r["score2"])
    r["s1"], r["s1_near"] = ref_step1(r["base"])
    r["s2"], r["secs"] = ref_step2(r["s1"])
    r["ext"], r["ext_margins"] = ref_extend(r["s2"], r["secs"], r["cand2"], r["score2"])
    r["kept"], r["order"], r["s3"], r["ms"], r["trace"] = ref_merge(r["ext"], r["s2"], r["cand2"], r["score2"])
    r["s4"], r["final"] = ref_bridge(r["s3"])
    r["sm"] = ref_smooth(r["s4"])
    r["out"] = ref_sample(r["sm"], d["nout"], frame_period, zero_below)
    return r


def exclusions(r):
    """-> {stage: (excluded, elements)} of the elementwise gates of a chain (or of the child's teacher-forced stages)."""
    return {k: (int(r[k + "_near"].sum()), int(r[k + "_near"].size)) for k in ("raw", "refine", "reliable", "s1")}


def steering_margins(r):
    """-> the steering decisions of a chain that lie inside the margin band (must be empty)."""
    bad = []
    if (r["hlen_margin"] < MARGIN).any():
        bad.append("hlen")
    if any(m < MARGIN for m in r["ext_margins"]):
        bad.append("extension / keep")
    if merge_margins(r["trace"]):
        bad.append("merge score sums")
    return bad


def smoother_cuts(final, nfr, marg=600):
    """-> per final section (cut below?, cut above?) as hv_smooth_kernel decides it."""
    return [(st - marg > -300, ed + marg < nfr + 299) for st, ed in final]
