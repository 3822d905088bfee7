"""GPU child: Harvest f0 (csrc/harvest.hip) stage by stage against oracle/f0_ref.py, at the edges tests/harvest_oracle.py lists.

One run of this file computes every case on the device through the C entry, reads the workspace back through
knnsvc_debug_f0_harvest_layout, and notes one entry per (case, stage): ``stage/<case>/<stage>``.

  teacher forcing   stage s of the device is compared with the oracle's stage s applied to the DEVICE's output of stage s - 1
                    (read back as fp64).  The full oracle run from the waveform is compared as well (``track``), with the bound
                    tests/test_gpu_f0.py uses: voicing agreement >= 0.99 and 1e-3 Hz on >= 99 % of the frames voiced in both.
  value stages      decimate, bank, refine/pitch, refine/deviation (1 / score, the quantity computed), smooth:
                    max |device - reference| over the stage divided by the stage's largest |reference| <= BARS[stage]; the bars
                    are eight times the worst error measured on the MI355X over all cases, rounded up to a power of ten, and
                    none is above 1e-9 (profiles/harvest_errors.txt).  mean: within ylen * 2^-53 * max |y| of math.fsum.
  decision stages   everything else: integer results (event counts, hlen, section bounds, kept sections, merge order, info,
                    status) equal; the zero pattern of every array equal; values within 2^-40 relative.  A gate inside the
                    margin band (1e-9 of its threshold in the oracle) is excluded and takes the device's value; at most 0.1 % of
                    a stage's elements per case.  The steering decisions (hlen, every selection of the extension, the kept
                    sections, the merge order and steps) allow none: their margins are asserted on the oracle, fed with the
                    device's inputs, BEFORE the device's output is looked at.
  workspace         natural, dense, merge: the same input twice in one workspace, filled with 0x00 and then 0xFF: every written
                    array, the track and status bit-identical; the padding between the arrays and the guard bytes around the
                    workspace still 0xFF; high-water marks of the fixed capacities in the detail.
  args              the smallest and the largest floor the entry serves (both entries and the layout agree, one message), n_frames
                    off by one, a workspace one byte short or off its alignment: an error, the output untouched."""
import ctypes
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle import f0_ref                                        # noqa: E402
from tests import harvest_oracle as O                            # noqa: E402
from tests.gpu_child import DEV, REPORT, note, run_cases         # noqa: E402

GUARD = 4096
# value stages: eight times the worst error measured on the MI355X over all cases, rounded up to a power of ten (measured: decimate
# 6.5e-16, bank 3.0e-15, refine/pitch 1.1e-14, refine/deviation 3.1e-11, smooth 5.6e-15; profiles/harvest_errors.txt).  The
# deviation weighs every harmonic alike, so it carries the FFT's error at the weakest harmonic's bin (some 1e-16 of the strongest
# bin, divided by the weak bin's power) where the pitch weighs by amplitude: the reference's error, and still under the 1e-9 cap.
BARS = {"decimate": 1e-14, "bank": 1e-13, "refine/pitch": 1e-13, "refine/deviation": 1e-9, "smooth": 1e-13}
WORST = {}                    # stage -> (worst figure, case)
EXCLUDED = {}                 # stage -> (largest share excluded, case)


def _lib():
    from knn_svc_amd import _lib
    lib = _lib.load()
    lib.knnsvc_debug_f0_harvest_layout.restype = ctypes.c_int32
    lib.knnsvc_debug_f0_harvest_layout.argtypes = [ctypes.c_int64, ctypes.c_int32, ctypes.c_float, ctypes.c_float, ctypes.c_float,
                                                   ctypes.POINTER(ctypes.c_int64), ctypes.c_int32]
    return lib


def last_error(lib):
    return lib.knnsvc_last_error().decode("utf-8", "replace")


def layout(lib, L, f0_floor, f0_ceil, frame_period):
    """-> (return code, {array: (offset, bytes)}, {dimension: value})"""
    table = (ctypes.c_int64 * O.N_TABLE)()
    rc = lib.knnsvc_debug_f0_harvest_layout(L, O.FS, f0_floor, f0_ceil, frame_period, table, O.N_TABLE)
    return (rc, *O.parse_layout(table)) if rc == 0 else (rc, None, None)


def workspace_size(lib, L, f0_floor, f0_ceil, frame_period):
    n, nbytes = ctypes.c_int64(-1), ctypes.c_int64(-1)
    rc = lib.knnsvc_f0_harvest_workspace(L, O.FS, f0_floor, f0_ceil, frame_period, ctypes.byref(n), ctypes.byref(nbytes))
    return rc, n.value, nbytes.value


def call(lib, x, params, out, n_frames, ws_ptr, ws_bytes, status):
    from knn_svc_amd import ops
    f0_floor, f0_ceil, frame_period, zero_below = params
    return lib.knnsvc_f0_harvest(ops._p(x), x.numel(), O.FS, f0_floor, f0_ceil, frame_period, zero_below, ops._p(out), n_frames,
                                 ctypes.c_void_p(ws_ptr), ws_bytes, ops._p(status), ops._stream())


class Run:
    """One call of the C entry in a workspace filled with ``fill``, guard bytes around it -> the workspace on the host."""
    def __init__(self, lib, x32, params, fill, buf=None):
        L = len(x32)
        rc, self.arr, self.d = layout(lib, L, *params[:3])
        assert rc == 0, last_error(lib)
        rc, nout, nbytes = workspace_size(lib, L, *params[:3])
        assert rc == 0 and nout == self.d["nout"] and nbytes == self.d["total"], (rc, nout, nbytes, self.d)
        self.buf = buf if buf is not None else torch.empty(nbytes + 2 * GUARD, device=DEV, dtype=torch.uint8)
        assert self.buf.data_ptr() % 256 == 0 and self.buf.numel() == nbytes + 2 * GUARD
        self.buf.fill_(fill)
        x = torch.from_numpy(x32).to(DEV)
        out = torch.full((nout + 128,), -7.25e11, device=DEV)
        status = torch.full((1,), -1, device=DEV, dtype=torch.int32)
        rc = call(lib, x, params, out[64:64 + nout], nout, self.buf.data_ptr() + GUARD, nbytes, status)
        assert rc == 0, last_error(lib)
        torch.cuda.synchronize()
        host = self.buf.cpu().numpy()
        self.fill, self.nbytes = fill, nbytes
        self.guards_ok = bool((host[:GUARD] == fill).all() and (host[GUARD + nbytes:] == fill).all())
        self.ws = host[GUARD:GUARD + nbytes]
        o = out.cpu().numpy()
        self.out_guards_ok = bool((o[:64] == np.float32(-7.25e11)).all() and (o[64 + nout:] == np.float32(-7.25e11)).all())
        self.out = o[64:64 + nout].copy()
        self.status = int(status.item())
        d = self.d
        shapes = {"filt": (d["nch"], d["ld"]), "events": (d["nch"], 4, d["ecap"]), "ecount": (d["nch"], 4), "raw": (d["nch"], d["nfr"]),
                  "cand0": (d["nfr"], O.NC), "cand": (d["nfr"], O.NS), "score": (d["nfr"], O.NS), "cand2": (d["nfr"], O.NS),
                  "score2": (d["nfr"], O.NS)}
        self.v = {}
        for name, dt in O.ARRAYS:
            off, size = self.arr[name]
            a = self.ws[off:off + size].view(dt)
            self.v[name] = a.reshape(shapes[name]) if name in shapes else a

    def written(self):
        """-> {name: the part of each array that the run writes and a later stage (or the caller) reads}."""
        v, d = self.v, self.d
        n2, nk, _, n4 = (int(i) for i in v["info"][:4])
        used = int(v["woff"][n2])
        w = {k: v[k] for k in ("t1", "t2", "mean", "ypad", "bf0", "hlen", "ecount", "raw", "cand0", "cand", "score", "cand2", "score2",
                               "base", "s1", "s2", "s3", "s4", "sm")}
        w["filt"] = v["filt"][:, :d["ylen"]]
        w["events"] = np.concatenate([v["events"][c, k, :v["ecount"][c, k]] for c in range(d["nch"]) for k in range(4)])
        w.update(st=v["st"][:n2], ed=v["ed"][:n2], xst=v["xst"][:n2], xed=v["xed"][:n2], keep=v["keep"][:nk], order=v["order"][:nk],
                 gst=v["gst"][:n4], ged=v["ged"][:n4], woff=v["woff"][:n2 + 1], soff=v["soff"][:n4], chan=v["chan"][:used],
                 chs=v["chs"][:used], info=v["info"][:4], out=self.out)
        if nk:
            w["ms"] = v["ms"]
        return w

    def gaps_ok(self):
        """The padding behind every array still holds the fill byte -> the names of the arrays whose padding does not."""
        names = [n for n, _ in O.ARRAYS]
        ends = [self.arr[n][0] for n in names[1:]] + [self.nbytes]
        return [n for n, e in zip(names, ends) if not (self.ws[sum(self.arr[n]):e] == self.fill).all()]


# ------------------------------------------------------------------ comparisons
def worst(table, stage, figure, case):
    if stage not in table or figure > table[stage][0]:
        table[stage] = (figure, case)


def value_stage(case, stage, dev, ref, on=None):
    """max |device - reference| / max |reference| against BARS[stage]; on: the elements compared."""
    if on is not None:
        dev, ref = dev[on], ref[on]
    scale = float(np.abs(ref).max()) if ref.size else 0.0
    diff = float(np.abs(dev - ref).max()) if ref.size else 0.0
    err = diff / scale if scale > 0 else (0.0 if diff == 0 else np.inf)
    if not np.isfinite(err):
        err = np.inf
    worst(WORST, stage, err, case)
    note(f"stage/{case}/{stage}", err <= BARS[stage], f"error {err:.3g} of the largest |reference| {scale:.6g}, bar {BARS[stage]:g}, {ref.size} elements")


def decision(case, stage, pairs, ints=(), near=None, extra=""):
    """pairs: (name, device, reference) float arrays; ints: (name, device, reference) that must be equal; near: a mask over the
    FIRST pair's shape of the gates inside the margin band (those elements of every same-shaped pair take the device's value)."""
    bad, rel_worst, nex, size = [], 0.0, 0, 0
    for name, dv, rf in ints:
        dv, rf = np.atleast_1d(dv), np.atleast_1d(rf)
        if dv.shape != rf.shape or not np.array_equal(dv, rf):
            bad.append(f"{name}: {dv.tolist()[:12]} != {rf.tolist()[:12]}" if dv.size < 400 else f"{name} differs")
    for name, dv, rf in pairs:
        dv, rf = np.asarray(dv, np.float64), np.asarray(rf, np.float64)
        if dv.shape != rf.shape:
            bad.append(f"{name}: shape {dv.shape} != {rf.shape}")
            continue
        if near is not None and near.shape == rf.shape:
            rf = np.where(near, dv, rf)
        if not np.isfinite(dv).all():
            bad.append(f"{name}: {int((~np.isfinite(dv)).sum())} non-finite values")
            continue
        pat = (dv != 0) != (rf != 0)
        if pat.any():
            bad.append(f"{name}: zero pattern differs at {int(pat.sum())} elements, first {np.argwhere(pat)[0].tolist()}")
        big = np.maximum(np.abs(dv), np.abs(rf))
        rel = np.where(big > 0, np.abs(dv - rf) / np.where(big > 0, big, 1), 0.0)
        rel[pat] = 0
        if rel.size:
            rel_worst = max(rel_worst, float(rel.max()))
            if rel.max() > O.VALUE_TOL:
                bad.append(f"{name}: {int((rel > O.VALUE_TOL).sum())} values off by up to {rel.max():.3g} relative")
    if near is not None:
        nex, size = int(near.sum()), int(near.size)
        if nex > O.CAP * size:
            bad.append(f"{nex} of {size} elements inside the margin band: over the cap")
        worst(EXCLUDED, stage, nex / max(size, 1), case)
    worst(WORST, stage, rel_worst, case)
    note(f"stage/{case}/{stage}", not bad, "; ".join(bad) if bad else f"worst value difference {rel_worst:.3g} relative, {nex} of {size} excluded{extra}")


def agreement(f, r):
    f, r = np.asarray(f, np.float64), np.asarray(r, np.float64)
    vf, vr = f > 0, r > 0
    both = vf & vr
    return float((vf == vr).mean()), np.abs(f[both] - r[both])


# ------------------------------------------------------------------ one case, every stage
def stages(case, x32, params, run):
    f0_floor, f0_ceil, frame_period, zero_below = params
    v, d = run.v, run.d
    L, ylen, nfr, nch = len(x32), d["ylen"], d["nfr"], d["nch"]
    want = O.dims(L, f0_floor, f0_ceil, frame_period)
    assert all(d[k] == want[k] for k in want), (d, want)
    pad = d["HV_YPAD"]

    dec = v["t2"][2 - 2 * ylen + L + 8 + 2 * np.arange(ylen)]
    value_stage(case, "decimate", dec, O.ref_decimate(x32))

    mean, bound = O.ref_mean(dec)
    err = abs(float(v["mean"][0]) - mean)
    worst(WORST, "mean", err / bound if bound else 0.0, case)
    note(f"stage/{case}/mean", err <= bound, f"|mean - fsum mean| {err:.3g}, bound ylen * 2^-53 * max |y| = {bound:.3g}")
    y = v["ypad"][pad:pad + ylen]
    note(f"stage/{case}/centre", np.array_equal(y, dec - v["mean"][0]) and not v["ypad"][:pad].any() and not v["ypad"][pad + ylen:].any()
         and len(v["ypad"]) == ylen + 2 * pad, "ypad = decimated - mean between HV_YPAD zeros, bit for bit")

    hl, hmargin = O.ref_hlen(v["bf0"])
    assert (hmargin >= O.MARGIN).all(), "hlen: a rounding inside the margin band (steering: none allowed)"
    decision(case, "channels", [("bf0", v["bf0"], O.ref_channels(f0_floor, nch))], [("hlen", v["hlen"], hl)])

    value_stage(case, "bank", v["filt"][:, :ylen], O.ref_bank(y, v["bf0"]))

    ev = O.ref_events(v["filt"][:, :ylen])
    counts = np.array([[len(e) for e in ch] for ch in ev])
    dev_ev = [[v["events"][c, k, :v["ecount"][c, k]] for k in range(4)] for c in range(nch)]
    flat = lambda lists: np.concatenate([e for ch in lists for e in ch] + [np.zeros(0)])
    ff = v["filt"][:, :ylen]
    dd = np.diff(ff, axis=1)                      # events that the `<= 0` side of the test decides: an exact 0 after a value off it
    exact = int(((ff[:, :-1] != 0) & (ff[:, 1:] == 0)).sum() + ((dd[:, :-1] != 0) & (dd[:, 1:] == 0)).sum())
    decision(case, "events", [("positions", flat(dev_ev), flat(ev))] if np.array_equal(counts, v["ecount"]) else [],
             [("counts", v["ecount"], counts)], extra=f", largest count {int(counts.max())} of ecap {d['ecap']}, {exact} events at an exact zero")

    raw, near = O.ref_raw(dev_ev, v["bf0"], f0_floor, f0_ceil, nfr)
    decision(case, "raw", [("raw", v["raw"], raw)], near=near)

    decision(case, "candidates", [("cand0", v["cand0"], O.ref_detect(v["raw"]))], extra=f", up to {int((v['cand0'] > 0).sum(1).max())} per frame")

    rf, sc, _urf, _dev, near = O.ref_refine(y, v["cand0"], f0_floor, f0_ceil)
    both = (v["cand"] != 0) & (rf != 0)
    value_stage(case, "refine/pitch", v["cand"], rf, both)
    with np.errstate(divide="ignore"):
        value_stage(case, "refine/deviation", 1.0 / v["score"], 1.0 / sc, both)
    decision(case, "refine/gates", [("cand", v["cand"] != 0, rf != 0), ("score", v["score"] != 0, sc != 0)], near=near,
             extra=f", {int(both.sum())} refined candidates")

    c2, s2c, near = O.ref_reliable(v["cand"], v["score"])
    decision(case, "reliable", [("cand2", v["cand2"], c2), ("score2", v["score2"], s2c)], near=near)

    decision(case, "base", [], [("base", v["base"], O.ref_base(v["cand2"], v["score2"]))])
    s1, near = O.ref_step1(v["base"])
    decision(case, "step1", [("s1", v["s1"], s1)], near=near)
    s2, secs = O.ref_step2(v["s1"])
    n2, nk, flags, n4 = (int(i) for i in v["info"][:4])
    decision(case, "step2", [("s2", v["s2"], s2)], [("sections", n2, len(secs)), ("st", v["st"][:n2], [s[0] for s in secs]),
                                                    ("ed", v["ed"][:n2], [s[1] for s in secs])], extra=f", {n2} sections of scap {d['scap']}")

    # extension: the oracle on the device's s2 / sections / candidates; its margins first
    dsecs = list(zip(v["st"][:n2].tolist(), v["ed"][:n2].tolist()))
    ext, margins = O.ref_extend(v["s2"], dsecs, v["cand2"], v["score2"])
    assert all(m >= O.MARGIN for m in margins), "extension: a selection or keep decision inside the margin band (steering: none allowed)"
    marg = d["HV_MARG"]
    win = [(max(st - marg, 0), min(ed + marg, nfr - 1)) for st, ed in dsecs]
    spans = np.array([0] + [we - ws + 1 for ws, we in win]).cumsum()
    chan = [v["chan"][o:o + we - ws + 1] for o, (ws, we) in zip(spans, win)]
    chs = [v["chs"][o:o + we - ws + 1] for o, (ws, we) in zip(spans, win)]
    cat = lambda parts: np.concatenate(list(parts) + [np.zeros(0)])
    kept = [k for k, e in enumerate(ext) if e[3]]
    outside = [bool(e[2][:ws].any() or e[2][we + 1:].any()) for e, (ws, we) in zip(ext, win)]
    decision(case, "extend", [("chan", cat(chan), cat(e[2][ws:we + 1] for e, (ws, we) in zip(ext, win))),
                              ("chs", cat(chs), cat(e[4][ws:we + 1] for e, (ws, we) in zip(ext, win)))],
             [("woff", v["woff"][:n2 + 1], spans), ("xst", v["xst"][:n2], [e[0] for e in ext]), ("xed", v["xed"][:n2], [e[1] for e in ext]),
              ("kept sections", v["keep"][:nk], kept), ("info[1]", nk, len(kept)), ("a channel beyond its window", outside, [False] * n2)],
             extra=f", {nk} of {n2} sections kept")

    # merge: the oracle on the device's channels, bounds and kept sections
    def full(part, k):
        a = np.zeros(nfr); a[win[k][0]:win[k][1] + 1] = part[k]
        return a
    dkept = v["keep"][:nk].tolist()
    dext = [(int(v["xst"][k]), int(v["xed"][k]), full(chan, k), k in dkept, None) for k in range(n2)]
    _, order, s3, ms, trace = O.ref_merge(dext, v["s2"], v["cand2"], v["score2"])
    assert not O.merge_margins(trace), "merge: score sums inside the margin band (steering: none allowed)"
    br = [s["branch"] for s in trace["steps"]]
    decision(case, "merge", [("s3", v["s3"], s3)] + ([("ms", v["ms"], ms)] if nk else []), [("order", v["order"][:nk], order)],
             extra=f", steps: {br.count('after')} after, {br.count('inside')} inside, {br.count('sum')} by score sum")

    s4, final = O.ref_bridge(v["s3"])
    decision(case, "bridge", [("s4", v["s4"], s4)], [("final sections", n4, len(final)), ("gst", v["gst"][:n4], [s[0] for s in final]),
                                                     ("ged", v["ged"][:n4], [s[1] for s in final])])
    value_stage(case, "smooth", v["sm"], O.ref_smooth(v["s4"]))

    sampled = O.ref_sample(v["sm"], d["nout"], frame_period, zero_below)
    ok = np.array_equal(sampled.view(np.uint32), run.out.view(np.uint32)) and run.status == 0 and flags == 0 and run.out_guards_ok
    if case == "low-70":
        ok = ok and not run.out.any() and (v["sm"] > 0).mean() > 0.9
    if case == "low-70-zero-0":
        ok = ok and (run.out > 0).mean() > 0.9 and (run.out[run.out > 0] < 80).all()
    note(f"stage/{case}/sample", ok, f"fp32 track = sm sampled, bit for bit; status {run.status}; {(run.out > 0).mean():.3f} voiced")

    track = f0_ref.harvest(x32.astype(np.float64), O.FS, f0_floor, f0_ceil, frame_period, zero_below)
    agree, diff = agreement(run.out, track)
    close = float((diff < 1e-3).mean()) if len(diff) else 1.0
    ok = len(track) == len(run.out) and agree >= 0.99 and close >= 0.99
    if case == "silence":
        ok = ok and not run.out.any()
    if case == "noise":
        ok = ok and (run.out > 0).mean() < 0.3
    note(f"stage/{case}/track", ok, f"voicing agreement {agree:.5f}, 1e-3 Hz on {close:.5f} of {len(diff)} frames voiced in both, "
                                   f"max {diff.max() if len(diff) else 0:.3g} Hz")
    return final


def marks(run, final):
    """How near the fixed capacities the run came."""
    v, d = run.v, run.d
    n2, nk, _, n4 = (int(i) for i in v["info"][:4])
    used = 0
    if n4:
        st, ed = final[n4 - 1]
        used = int(v["soff"][n4 - 1]) + (min(ed + d["HV_SMOOTH_MARG"], d["nfr"] + 299) - max(st - d["HV_SMOOTH_MARG"], -300) + 1)
    return (f"woff {int(v['woff'][n2])} / chan_cap {d['chan_cap']} = {int(v['woff'][n2]) / d['chan_cap']:.3f}; scratch {used} / scratch_cap "
            f"{d['scratch_cap']} = {used / d['scratch_cap']:.3f}; sections {n2} / scap {d['scap']} = {n2 / d['scap']:.3f}; "
            f"events {int(v['ecount'].max())} / ecap {d['ecap']} = {int(v['ecount'].max()) / d['ecap']:.3f}")


def case_stages():
    lib = _lib()
    for case in O.CASES:
        x32, params = O.wave(case)
        t0 = time.time()
        if case in O.WORKSPACE_CASES:
            first = Run(lib, x32, params, 0x00)
            run = Run(lib, x32, params, 0xFF, first.buf)
            a, b = first.written(), run.written()
            diff = [k for k in a if a[k].shape != b[k].shape or a[k].tobytes() != b[k].tobytes()]
            note(f"workspace/{case}/poison", not diff and first.status == run.status == 0,
                 f"0x00 against 0xFF fill: {len(a)} arrays bit-identical" if not diff else f"differ: {diff}")
            gaps = run.gaps_ok()
            note(f"workspace/{case}/gaps", not gaps, f"padding behind {len(O.ARRAYS)} arrays untouched" if not gaps else f"written: {gaps}")
            note(f"workspace/{case}/guard", run.guards_ok and first.guards_ok and run.out_guards_ok, f"{GUARD} bytes either side")
        else:
            run = Run(lib, x32, params, 0xFF)
        final = stages(case, x32, params, run)
        if case in O.WORKSPACE_CASES:
            note(f"workspace/{case}/marks", True, marks(run, final))
        print(f"     {case}: {time.time() - t0:.1f} s", flush=True)
    for stage, (fig, case) in sorted(WORST.items()):
        ex = f"; largest share excluded {EXCLUDED[stage][0]:.2e} ({EXCLUDED[stage][1]})" if stage in EXCLUDED else ""
        note(f"summary/{stage}", True, f"worst {fig:.3g} ({case}){ex}")


def case_args():
    lib = _lib()
    x32, _ = O.wave("min")
    L = len(x32)

    def accepts(f):
        return layout(lib, L, float(f), 1047.0, 20.0)[0] == 0
    lo, hi = np.float32(60.0), np.float32(70.0)
    assert not accepts(lo) and accepts(hi)
    while np.nextafter(lo, hi) < hi:
        mid = np.float32((float(lo) + float(hi)) / 2)
        lo, hi = (lo, mid) if accepts(mid) else (mid, hi)
    note("args/floor/smallest", hi == O.smallest_floor(), f"the layout entry accepts {float(hi):.7g} and up; the tile arithmetic says {float(O.smallest_floor()):.7g}")
    top = np.nextafter(np.float32(1600.0), np.float32(0.0))
    for name, (floor, ceil) in {"smallest": (float(hi), 1047.0), "largest": (float(top), 1600.0)}.items():
        params = (floor, ceil, 20.0, 0.0)
        run = Run(lib, x32, params, 0xFF)
        track = f0_ref.harvest(x32.astype(np.float64), O.FS, *params)
        agree, diff = agreement(run.out, track)
        close = float((diff < 1e-3).mean()) if len(diff) else 1.0
        note(f"args/floor/{name}/served", run.status == 0 and run.guards_ok and agree >= 0.99 and close >= 0.99,
             f"floor {floor:.7g}, ceil {ceil:g}, {run.d['nch']} channels: agreement {agree:.4f}, {len(diff)} voiced in both, 1e-3 Hz on {close:.4f}")

    x = torch.from_numpy(x32).to(DEV)
    rc, nout, nbytes = workspace_size(lib, L, *O.DEFAULT[:3])
    assert rc == 0
    ws = torch.zeros(nbytes + 512, device=DEV, dtype=torch.uint8)
    assert ws.data_ptr() % 256 == 0

    def refused(key, params, n_frames, ptr, nb, word):
        out = torch.full((nout + 2,), -7.25e11, device=DEV)
        status = torch.full((1,), -1, device=DEV, dtype=torch.int32)
        rc = call(lib, x, params, out, n_frames, ptr, nb, status)
        msg = last_error(lib)
        torch.cuda.synchronize()
        note(f"args/{key}", rc != 0 and word in msg and bool((out == -7.25e11).all()) and int(status.item()) == -1, f"rc {rc}: {msg}")
    below = float(np.nextafter(hi, np.float32(0.0)))
    low = (below, 1047.0, 20.0, 80.0)
    refused("floor/below/run", low, nout, ws.data_ptr(), nbytes, "f0_floor too low")
    rc_w = workspace_size(lib, L, *low[:3])[0]
    msg_w = last_error(lib)
    rc_l = layout(lib, L, *low[:3])[0]
    msg_l = last_error(lib)
    note("args/floor/below/workspace", rc_w != 0 and rc_l != 0 and msg_w == msg_l and "f0_floor too low" in msg_w, f"rc {rc_w}, {rc_l}: {msg_w}")
    refused("floor/at-ceil", (1047.0, 1047.0, 20.0, 80.0), nout, ws.data_ptr(), nbytes, "bad range")
    refused("n_frames/minus-1", O.DEFAULT, nout - 1, ws.data_ptr(), nbytes, "n_frames")
    refused("n_frames/plus-1", O.DEFAULT, nout + 1, ws.data_ptr(), nbytes, "n_frames")
    refused("workspace/one-byte-short", O.DEFAULT, nout, ws.data_ptr(), nbytes - 1, "workspace")
    refused("workspace/misaligned", O.DEFAULT, nout, ws.data_ptr() + 128, nbytes, "aligned")


if __name__ == "__main__":
    t0 = time.time()
    rc = run_cases([("stages", case_stages), ("args", case_args)], sys.argv[1])
    print(f"child wall time {time.time() - t0:.1f} s, {len(REPORT)} entries")
    sys.exit(rc)
