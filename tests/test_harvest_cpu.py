"""CPU: what tests/harvest_child.py relies on, shown without a GPU.
  case generators   deterministic, of the stated length, and each reaches what it is there for (conditions on the oracle's
                    intermediates, so that a later change of a generator cannot quietly empty a case)
  staged references chained from the waveform they restate oracle/f0_ref.harvest bit for bit, for every case and parameter set
  margins           the oracle alone stays inside the exclusion caps: at most 0.1 % of a stage's gates within 1e-9 of their
                    threshold, none of the steering decisions
  layout entry      knnsvc_debug_f0_harvest_layout (host only): offsets ascending and 256-aligned inside what
                    knnsvc_f0_harvest_workspace reports, the oracle's dimensions for every parameter set, and the floors it
                    serves: the bank tile's bound at the low end, the ceiling at the high end"""
import ctypes
import functools

import numpy as np
import pytest

from oracle import f0_ref
from tests import harvest_oracle as O


@functools.lru_cache(maxsize=None)
def _chain(case):
    x, params = O.wave(case)
    return O.chain(x, params)


def _lib():
    import __graft_entry__ as g
    g.build()
    from knn_svc_amd import _lib
    lib = _lib.load()
    lib.knnsvc_debug_f0_harvest_layout.restype = ctypes.c_int32
    lib.knnsvc_debug_f0_harvest_layout.argtypes = [ctypes.c_int64, ctypes.c_int32, ctypes.c_float, ctypes.c_float, ctypes.c_float,
                                                   ctypes.POINTER(ctypes.c_int64), ctypes.c_int32]
    return lib


def _layout(lib, L, f0_floor, f0_ceil, frame_period, n=O.N_TABLE):
    table = (ctypes.c_int64 * O.N_TABLE)()
    rc = lib.knnsvc_debug_f0_harvest_layout(L, O.FS, f0_floor, f0_ceil, frame_period, table, n)
    return rc, table


def _workspace(lib, L, f0_floor, f0_ceil, frame_period):
    n, nbytes = ctypes.c_int64(-1), ctypes.c_int64(-1)
    rc = lib.knnsvc_f0_harvest_workspace(L, O.FS, f0_floor, f0_ceil, frame_period, ctypes.byref(n), ctypes.byref(nbytes))
    return rc, n.value, nbytes.value


# ------------------------------------------------------------------ case generators
@pytest.mark.parametrize("gen", sorted(O.GENERATORS))
def test_generators_are_deterministic_and_of_the_stated_length(gen):
    n, fn = O.GENERATORS[gen]
    a, b = np.asarray(fn(), np.float32), np.asarray(fn(), np.float32)
    assert a.shape == (n,) and np.array_equal(a, b) and np.isfinite(a).all() and np.abs(a).max() <= 1.0
    assert n <= 24077                                                           # 1.5 s: the oracle costs about a second per second


def test_case_lengths_sit_on_the_edges_they_are_named_for():
    L = {k: v[0] for k, v in O.GENERATORS.items()}
    assert L["min"] == 1600 and O.dims(1600, 65.0, 1047.0, 20.0) == {"nch": 172, "ylen": 800, "nfr": 101, "nout": 6}
    assert ((L["tile-1024"] - 1) // 2 + 1, (L["tile-1025"] - 1) // 2 + 1) == (1024, 1025)         # one bank tile; one sample into the second
    assert (2 - 2 * 1024 + L["tile-1024"], 2 - 2 * 1025 + L["tile-1025"]) == (2, 1)                # nbeg: even and odd L
    assert (L["chunk-4078"] + 18, L["chunk-4079"] + 18) == (64 * 64, 64 * 64 + 1)                 # IIR chunks
    assert max(O.dims(24000, *p[:3])["nch"] for _, p in O.CASES.values()) == 197
    assert O.dims(24000, 100.0, 500.0, 1.0)["nout"] == O.dims(24000, 100.0, 500.0, 1.0)["nfr"] == 1501
    assert (np.arange(O.dims(24000, 65.0, 1047.0, 12.5)["nout"]) * 12.5 % 1 == 0.5).any()        # sample positions that end in .5


# ------------------------------------------------------------------ the chain restates the oracle; margins
@pytest.mark.parametrize("case", sorted(O.CASES))
def test_chained_stages_restate_the_oracle_bit_for_bit_inside_the_margin_caps(case):
    x, params = O.wave(case)
    r = _chain(case)
    want = f0_ref.harvest(x.astype(np.float64), O.FS, *params)
    assert want.shape == r["out"].shape == (r["nout"],)
    assert np.array_equal(want.astype(np.float32).view(np.uint32), r["out"].view(np.uint32))
    idx = np.minimum(r["nfr"] - 1, f0_ref._round(np.arange(r["nout"]) * params[2] / 1000.0 * 1000.0))
    sm = r["sm"][idx]
    assert np.array_equal(np.where(sm < params[3], 0.0, sm), want)                    # the fp64 track itself, not only its rounding
    for stage, (n, size) in O.exclusions(r).items():
        assert n <= O.CAP * size, (stage, n, size)
    assert O.steering_margins(r) == []


# ------------------------------------------------------------------ every case reaches what its row says
def _cuts(case):
    r = _chain(case)
    return set(O.smoother_cuts(r["final"], r["nfr"]))


def _branches(case):
    return [s["branch"] for s in _chain(case)["trace"]["steps"]]


def test_min_is_one_section_extended_to_both_ends_of_the_track_with_both_smoother_ends_uncut():
    """The extension stops at frames 1 and nfr - 2 and writes one frame past each: the section reaches frames 0 and nfr - 1.
    (Step 1 leaves frames 0 and 1 unvoiced, so no section STARTS at frame 1 before the extension; natural's last one ends at
    nfr - 2.)"""
    r = _chain("min")
    assert r["nfr"] == 101 and len(r["secs"]) == 1 and (r["ext"][0][0], r["ext"][0][1]) == (0, r["nfr"] - 1)
    assert _cuts("min") == {(False, False)} and (r["out"] > 0).all()
    n = _chain("natural")
    assert n["secs"][-1][1] == n["nfr"] - 2


@pytest.mark.parametrize("case", ["tile-1024", "tile-1025", "chunk-4078", "chunk-4079", "dc"])
def test_tone_cases_are_voiced_throughout(case):
    r = _chain(case)
    assert len(r["secs"]) >= 1 and (r["out"] > 0).all() and r["final"] == [(0, r["nfr"] - 1)]


def test_natural_has_gaps_and_a_smoother_end_of_each_kind():
    r = _chain("natural")
    assert len(r["final"]) >= 2 and 0.5 < (r["out"] > 0).mean() < 0.95
    assert {(False, True), (True, False)} <= _cuts("natural")


def test_dense_has_dozens_of_sections_every_merge_branch_and_smoother_ends_cut_on_both_sides():
    r = _chain("dense")
    assert len(r["secs"]) >= 20 and len(r["kept"]) >= 20 and len(r["final"]) >= 6
    assert (True, True) in _cuts("dense")
    assert {"after", "inside", "sum"} <= set(_branches("dense"))


def test_merge_has_forty_sections_that_become_one_track_through_score_sums_and_insides():
    r = _chain("merge")
    assert len(r["secs"]) >= 40 and len(r["final"]) == 1
    assert _branches("merge").count("sum") >= 30 and _branches("merge").count("inside") >= 1
    sums = [s for s in r["trace"]["steps"] if s["branch"] == "sum"]
    assert any(s["sc1"] > s["sc2"] for s in sums) and any(not s["sc1"] > s["sc2"] for s in sums)      # both outcomes of the comparison


def test_two_voices_has_competing_candidates_and_weak_drops_a_section_by_the_2200_rule():
    r = _chain("two-voices")
    assert ((r["cand0"] > 0).sum(1) >= 3).mean() > 0.5 and len(r["final"]) >= 2 and (True, True) in _cuts("two-voices")
    w = _chain("weak")
    dropped = [e for e in w["ext"] if not e[3]]
    assert dropped and len(w["kept"]) >= 1 and all(e[1] - e[0] < 2200.0 / 65.0 for e in dropped)


def test_noise_and_silence_have_no_section_at_all():
    for case in ("noise", "silence"):
        r = _chain(case)
        assert r["secs"] == [] and r["kept"] == [] and r["final"] == [] and not r["out"].any() and not r["sm"].any()
    assert (_chain("noise")["cand0"] > 0).any()                                       # candidates, but no contour
    s = _chain("silence")
    assert not s["raw"].any() and all(len(e) == 0 for ch in s["events"] for e in ch)


def test_low_70_has_the_longest_windows_and_a_track_under_zero_below():
    r = _chain("low-70")
    c = r["cand0"][r["cand0"] > 0]
    n = 2 * (1.5 * 8000.0 / c + 1.0).astype(np.int64) + 1
    assert (n == 345).mean() > 0.1 and n.max() <= 384
    assert (r["sm"] > 0).mean() > 0.9 and (r["sm"][r["sm"] > 0] < 80).all() and not r["out"].any()
    z = _chain("low-70-zero-0")
    assert (z["out"] > 0).mean() > 0.9 and np.array_equal(z["sm"], r["sm"])


def test_params_cases_change_the_channel_count_and_the_sampling():
    assert _chain("params/80-1600-5")["nch"] == 185 and _chain("params/100-500-1")["nch"] == 105
    assert _chain("params/100-500-1")["nout"] == 1501 and _chain("params/65-1047-12.5")["nout"] == 121
    assert _chain("params/65-1600-20")["nch"] == 197
    for case in ("params/80-1600-5", "params/100-500-1", "params/65-1047-12.5", "params/65-1600-20"):
        assert (_chain(case)["out"] > 0).mean() > 0.2


# ------------------------------------------------------------------ the layout entry and the floors it serves
@pytest.mark.parametrize("case", sorted(O.CASES))
def test_layout_is_ascending_aligned_inside_the_workspace_and_has_the_oracles_dimensions(case):
    lib = _lib()
    gen, params = O.CASES[case]
    L = O.GENERATORS[gen][0]
    rc, table = _layout(lib, L, *params[:3])
    assert rc == 0
    arr, d = O.parse_layout(table)
    rc, nout, nbytes = _workspace(lib, L, *params[:3])
    assert rc == 0 and nout == d["nout"] and nbytes == d["total"]
    offs = [arr[name] for name, _ in O.ARRAYS]
    assert offs[0][0] == 0 and all(o % 256 == 0 and s > 0 for o, s in offs)
    assert all(a[0] + a[1] <= b[0] for a, b in zip(offs[:-1], offs[1:])) and offs[-1][0] + offs[-1][1] <= nbytes
    want = O.dims(L, *params[:3])
    assert {k: d[k] for k in want} == want
    assert (d["HV_NC"], d["HV_NS"], d["HV_YPAD"], d["HV_MARG"], d["HV_SMOOTH_MARG"]) == (O.NC, O.NS, 288, 104, 600)
    item = {"f8": 8, "i4": 4, "i8": 8}
    size = {"t1": L + 18, "t2": L + 18, "mean": 1, "ypad": d["ylen"] + 2 * d["HV_YPAD"], "bf0": d["nch"], "hlen": d["nch"],
            "filt": d["nch"] * d["ld"], "events": d["nch"] * 4 * d["ecap"], "ecount": d["nch"] * 4, "raw": d["nch"] * d["nfr"],
            "cand0": d["nfr"] * O.NC, "chan": d["chan_cap"], "chs": d["chan_cap"], "scratch": d["scratch_cap"], "woff": d["scap"] + 1,
            "soff": d["scap"] + 1, "info": 16}
    size.update({k: d["nfr"] * O.NS for k in ("cand", "score", "cand2", "score2")})
    size.update({k: d["nfr"] for k in ("base", "s1", "s2", "s3", "s4", "sm", "ms")})
    size.update({k: d["scap"] for k in ("st", "ed", "xst", "xed", "keep", "order", "gst", "ged")})
    assert {name: arr[name][1] for name, _ in O.ARRAYS} == {name: size[name] * item[dt] for name, dt in O.ARRAYS}
    assert d["ld"] >= d["ylen"] + 2 and d["ecap"] >= d["ylen"] // 2 and d["scap"] >= d["nfr"] // 2


def test_layout_refuses_a_short_table_and_what_the_run_refuses():
    lib = _lib()
    assert _layout(lib, 1600, 65.0, 1047.0, 20.0, O.N_TABLE - 1)[0] != 0
    assert b"f0_harvest_layout" in lib.knnsvc_last_error()
    assert _layout(lib, 1599, 65.0, 1047.0, 20.0)[0] != 0 and _workspace(lib, 1599, 65.0, 1047.0, 20.0)[0] != 0


def test_both_entries_serve_the_floors_the_bank_tile_serves_and_refuse_the_rest_with_one_message():
    lib = _lib()
    lo = O.smallest_floor()
    assert 64.5 < lo < 64.7
    below = np.nextafter(lo, np.float32(0.0))
    assert _layout(lib, 16000, float(lo), 1047.0, 20.0)[0] == 0 and _workspace(lib, 16000, float(lo), 1047.0, 20.0)[0] == 0
    msgs = []
    for fn in (_layout, _workspace):
        for f in (float(below), 64.0, 40.0, 1.0):
            assert fn(lib, 16000, f, 1047.0, 20.0)[0] != 0, f
            msgs.append(lib.knnsvc_last_error())
    assert set(msgs) == {b"f0_harvest: f0_floor too low"} or all(b"f0_floor too low" in m for m in msgs), msgs
    assert len({m for m in msgs}) == 1, msgs
    top = np.nextafter(np.float32(1600.0), np.float32(0.0))                          # the largest: just under the largest ceiling
    assert _layout(lib, 16000, float(top), 1600.0, 20.0)[0] == 0 and _workspace(lib, 16000, float(top), 1600.0, 20.0)[0] == 0
    for f, c in ((1600.0, 1600.0), (1047.0, 1047.0), (65.0, 1601.0), (0.0, 1047.0), (-65.0, 1047.0)):
        assert _layout(lib, 16000, f, c, 20.0)[0] != 0 and _workspace(lib, 16000, f, c, 20.0)[0] != 0, (f, c)
        assert b"bad range" in lib.knnsvc_last_error()
