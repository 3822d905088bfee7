"""CPU: harmony voices without a GPU — options.Harmony / HarmonyPart and matching.resolve_harmony, the oracle's own identities
(tests/harmony_oracle.py), the C ABI of knnsvc_harmony_f0_seg and knnsvc_mix_waves (every argument is checked before the launch, so
dummy pointers are never dereferenced), the command line, the entry points' refusals before a file is read, recording stand-ins
that show the defaults call the match functions as before, and the precondition of the GPU tests: every f0 case the GPU child
compares notes on stands at least 1e-6 semitone from every note decision going the other way."""
import ctypes
import dataclasses
import math
import os

import numpy as np
import pytest
import torch

import harmony_oracle as HO
import tune_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------- the oracle's own identities
def test_degree_move_in_c_major_gives_diatonic_thirds_and_sixths():
    m = O.mask_of("C:major")
    third = {60: 64, 62: 65, 64: 67, 65: 69, 67: 71, 69: 72, 71: 74}            # C-E (4), D-F (3), E-G (3), F-A (4), G-B (4), A-C (3), B-D (3)
    for n, t in third.items():
        assert HO.degree_move(m, n, 2)[0] == t and HO.degree_move(m, t, -2)[0] == n
    assert HO.degree_move(m, 60, -5)[0] == 52 and HO.degree_move(m, 60, 7) == (72, 1) and HO.degree_move(m, 60, -7) == (48, -1)
    assert HO.degree_move(m, 71, 1) == (72, 1) and HO.degree_move(m, 60, -1) == (59, -1)      # across the octave, both ways
    assert HO.degree_move(m, 60, 24)[0] == 60 + 36 + 5 and HO.degree_move(m, 60, -24)[0] == 60 - 48 + 7


def test_degree_move_floors_for_negative_notes_and_negative_indices():
    for scale in HO.MASKS + ("E:blues",):
        m = O.mask_of(scale)
        pcs = HO.degrees(m)
        d = len(pcs)
        allowed = [n for n in range(-40, 41) if (n % 12) in pcs]
        for s in range(-24, 25):
            for i, n in enumerate(allowed):
                t = HO.degree_move(m, n, s)[0]
                if 0 <= i + s < len(allowed):
                    assert t == allowed[i + s], (scale, n, s)                   # s places along the ladder of allowed notes
                assert HO.degree_move(m, n, d)[0] == n + 12 and HO.degree_move(m, n, -d)[0] == n - 12
        if scale == "chromatic":
            assert all(HO.degree_move(m, n, s)[0] == n + s for n in (-13, -1, 0, 5) for s in (-24, -1, 1, 24))


def test_oracle_chromatic_is_a_parallel_part_and_an_octave_is_an_octave():
    x = O.steps()
    for s in (3, -4, 24):
        y, t, D, pitched, _m = HO.harmony(x, [0, x.size], [HO.P("chromatic", s, 40.0)])
        assert np.array_equal(D[pitched], np.full(int(pitched.sum()), s)) and np.array_equal(y.view(np.uint32), HO.parallel(x, s).view(np.uint32))
        assert np.array_equal(y[~pitched].view(np.uint32), x[~pitched].view(np.uint32)) and bool((t[~pitched] == -1).all())
    for scale in HO.MASKS:
        d = len(HO.degrees(O.mask_of(scale)))
        up = HO.harmony(x, [0, x.size], [HO.P(scale, d, 189.8)])
        dn = HO.harmony(x, [0, x.size], [HO.P(scale, -d, 189.8)])
        p = up[3]
        assert bool((up[2][p] == 12).all()) and bool((dn[2][p] == -12).all())
        assert np.allclose(up[0][p] / x[p], 2.0, rtol=3e-7, atol=0) and np.allclose(dn[0][p] / x[p], 0.5, rtol=3e-7, atol=0)


def test_oracle_keeps_the_leads_deviation_and_glides_across_a_note_change():
    """Two notes of C major, 30 frames each, the lead 20 cents sharp with a vibrato: a third above is 4 semitones over C and 3 over
    D.  With a = 1 the interval jumps; with a = 0.1 it moves by a tenth of what is left per frame; the part is as sharp as the lead."""
    i = np.arange(30)
    x = O.hz(np.concatenate([60.2 + 0.3 * np.sin(i), 62.2 + 0.3 * np.sin(i)]))
    semis = lambda f: 69.0 + 12.0 * np.log2(f.astype(np.float64) / 440.0)
    y1, t1, D1, _p, _m = HO.harmony(x, [0, 60], [HO.P("C:major", 2, 0.0)])
    assert np.array_equal(D1, [4] * 30 + [3] * 30) and np.array_equal(t1, [64] * 30 + [65] * 30)
    assert np.allclose(semis(y1) - semis(x), D1, atol=2e-6)                     # the deviation from the note, to a fraction of a cent
    p = HO.P("C:major", 2, 189.8)
    y2, _t, D2, _p, _m = HO.harmony(x, [0, 60], [p])
    h = semis(y2) - semis(x)
    assert np.array_equal(D2, D1) and np.allclose(h[:30], 4.0, atol=2e-6)
    k = np.arange(1, 31)
    assert np.allclose(h[30:], 3.0 + (1.0 - p.alpha) ** k, atol=2e-6) and 0.09 < p.alpha < 0.11
    # a rest ends the run: the glide starts again at the new interval
    x3 = np.concatenate([x[:30], np.zeros(1, np.float32), x[30:]])
    y3 = HO.harmony(x3, [0, 61], [p])[0]
    assert np.allclose(semis(y3[31:]) - semis(x3[31:]), 3.0, atol=2e-6) and y3[30] == 0


def test_oracle_off_segments_and_mix():
    x = O.steps()[:100]
    for p in (None, HO.P("C:major", 0), HO.P_(0, 3, 1.0, math.log(440.0))):
        y, t, D, pitched, margin = HO.harmony(x, [0, 100], [p])
        assert np.array_equal(y.view(np.uint32), x.view(np.uint32)) and bool((t == -1).all()) and not pitched.any() and margin == np.inf
    a, b, c = (np.random.default_rng(s).standard_normal(50).astype(np.float32) for s in (1, 2, 3))
    nan = np.full(50, np.nan, np.float32)
    assert np.array_equal(HO.mix([a, nan, b], [0.5, 0.0, 0.25]), (0.5 * a.astype(np.float64) + 0.25 * b.astype(np.float64)).astype(np.float32))
    assert np.array_equal(HO.mix([a], [1.0]), a) and np.array_equal(HO.mix([a, b], [2.0, 0.0]), a + a)


def test_every_gpu_case_stands_clear_of_a_note_decision_and_covers_what_the_issue_lists():
    seen_d, seen_steps, seen_a, carries, negative = set(), set(), set(), set(), False
    for name, (f0, seg, parts) in HO.kernel_cases().items():
        assert seg[-1] == f0.size and len(parts) == len(seg) - 1
        for s, p in enumerate(parts):
            y, t, D, pitched, margin, q = HO.harmony_one(f0[seg[s]:seg[s + 1]], p)
            assert margin >= 1e-6, (name, s, margin)
            if p is None or p.steps == 0:
                continue
            d = len(HO.degrees(p.mask))
            seen_d.add(d); seen_steps.add(p.steps if abs(p.steps) in (1, 2, 24) else ("d" if p.steps == d else "-d" if p.steps == -d else p.steps))
            seen_a.add(round(p.alpha, 2))
            if abs(p.steps) < d:
                carries |= q
            negative = negative or bool((t[pitched] < 0).any() and ((t[pitched] - D[pitched]) < 0).any())
    assert {1, 5, 7, 12} <= seen_d and {1, -1, 2, -2, "d", "-d", 24, -24} <= seen_steps and {1.0, 0.39, 0.1} <= seen_a
    assert {-1, 0, 1} <= carries               # a degree move that crosses an octave upwards, and one downwards
    assert negative                            # notes below 0 (under 8.18 Hz) on both sides of the move
    f0, seg, parts = HO.kernel_cases()["one-run"]
    assert seg[1] == 1500 and bool((f0[:1500] > 0).all())
    assert len(HO.kernel_cases()["steps"][2]) == 96


# ---------------------------------------------------------------- the records
def test_harmony_defaults_and_derived_values():
    from knn_svc_amd.options import Harmony, HarmonyPart, HarmonyShift, SourceKnobs, Extensions, Tuning, TUNE_OFF
    h = Harmony((2, HarmonyPart(-3, -9.0)), scale="A:minor")
    assert h.parts == (HarmonyPart(2, -6.0), HarmonyPart(-3, -9.0)) and (h.lead_db, h.glide_ms, h.tuning_hz) == (0.0, 40.0, None)
    assert h.alpha == -math.expm1(-20.0 / 40.0) and Harmony(2, scale="chromatic", glide_ms=0).alpha == 1.0
    assert h.gains == (1.0, 10.0 ** (-6.0 / 20.0), 10.0 ** (-9.0 / 20.0))
    want = HO.P("A:minor", 2, 40.0)
    assert h.shifts() == (HarmonyShift(want.mask, 2, want.alpha, want.log_ref), HarmonyShift(want.mask, -3, want.alpha, want.log_ref))
    assert Harmony([2], scale="C:major") == Harmony((HarmonyPart(2),), scale="C:major") == Harmony(2, scale="C:major")
    # scale / tuning_hz None: the item's tune names them; a tune that is off counts as none; without either 440
    bare = Harmony((2,))
    assert bare.shifts(Tuning("G:major", tuning_hz=432.0)) == Harmony((2,), scale="G:major", tuning_hz=432.0).shifts()
    assert Harmony((2,), scale="C:major").shifts(Tuning("G:major", tuning_hz=432.0))[0].log_ref == math.log(432.0)
    assert Harmony((2,), scale="C:major").shifts()[0].log_ref == math.log(440.0)
    for t in (None, TUNE_OFF, Tuning("C:major", strength=0)):
        with pytest.raises(ValueError, match="scale"):
            bare.shifts(t)
    with pytest.raises(dataclasses.FrozenInstanceError):
        h.lead_db = 1.0
    # the pinned records keep their fields: the part's record travels beside them
    assert [f.name for f in dataclasses.fields(SourceKnobs)][-1] == "tune" and "harmony" not in [f.name for f in dataclasses.fields(Extensions)]
    assert HarmonyShift(1, 2, 1.0, 0.0).on and not HarmonyShift(0, 2, 1.0, 0.0).on and not HarmonyShift(1, 0, 1.0, 0.0).on


@pytest.mark.parametrize("kw", [
    dict(parts=()), dict(parts=(1, 2, 3, 4)), dict(parts=(0,)), dict(parts=(25,)), dict(parts=(-25,)), dict(parts=(1.5,)), dict(parts=(True,)),
    dict(parts=("2",)), dict(parts="2,3"), dict(parts=None), dict(parts=(2,), scale="H:major"), dict(parts=(2,), scale="C:000000000000"),
    dict(parts=(2,), scale=5), dict(parts=(2,), lead_db=-60.5), dict(parts=(2,), lead_db=12.5), dict(parts=(2,), lead_db=float("nan")),
    dict(parts=(2,), lead_db="0"), dict(parts=(2,), glide_ms=-1), dict(parts=(2,), glide_ms=2000.5), dict(parts=(2,), glide_ms=True),
    dict(parts=(2,), tuning_hz=399), dict(parts=(2,), tuning_hz=481), dict(parts=(2,), tuning_hz="440")])
def test_harmony_refuses(kw):
    from knn_svc_amd.options import Harmony
    with pytest.raises(ValueError):
        Harmony(**kw)


@pytest.mark.parametrize("kw", [dict(steps=0), dict(steps=25), dict(steps=2.0), dict(steps=None), dict(steps=2, gain_db=-61), dict(steps=2, gain_db=12.1),
                                dict(steps=2, gain_db=float("inf")), dict(steps=2, gain_db=None), dict(steps=2, gain_db=False)])
def test_harmony_part_refuses(kw):
    from knn_svc_amd.options import HarmonyPart
    with pytest.raises(ValueError):
        HarmonyPart(**kw)


def test_resolve_harmony():
    from knn_svc_amd import matching as M
    from knn_svc_amd.options import Harmony
    h = Harmony((2,), scale="C:major")
    assert M.resolve_harmony(None) is None and M.resolve_harmony(h) is h and M.resolve_harmony("off") == M.HARMONY_OFF == M.resolve_harmony(" OFF ")
    assert M.resolve_harmony(h, 3) == [h, h, h] and M.resolve_harmony(None, 2) == [None, None]
    assert M.resolve_harmony([h, None, "off"], 3) == [h, None, M.HARMONY_OFF]
    for bad in (2, "C:major", (2,), True, 0.5):
        with pytest.raises(ValueError):
            M.resolve_harmony(bad) if not isinstance(bad, tuple) else M.resolve_harmony(bad, 2)
    for bad in ([h], [h, h, h], [h, 3]):
        with pytest.raises(ValueError):
            M.resolve_harmony(bad, 2)
    with pytest.raises(ValueError):
        M.resolve_harmony([h])
    assert M.harmony_of(None) is None and M.harmony_of(M.HARMONY_OFF) is None and M.harmony_of(h) == (h, h.shifts())


# ---------------------------------------------------------------- the C ABI
def _lib():
    import __graft_entry__ as g
    g.build()
    from knn_svc_amd import _lib
    return _lib.load()


def _table(lens):
    seg = [0]
    for n in lens:
        seg.append(seg[-1] + n)
    return (ctypes.c_int64 * len(seg))(*seg)


_f64 = lambda v: (ctypes.c_double * len(v))(*v)
_i32 = lambda v: (ctypes.c_int32 * len(v))(*v)


def test_harmony_f0_seg_refuses_bad_arguments_before_launching():
    lib = _lib()
    d, e = 256, 512              # dummies, aligned, never dereferenced: every call below fails before the launch
    seg = _table([3, 4])
    lr = math.log(440.0)
    ok = dict(mask=[0xFFF, 0], steps=[2, 0], alpha=[0.25, 1.0], log_ref=[lr, lr])
    big = 1 << 20

    def call(f0=d, table=seg, n=2, out=e, notes=None, ws=d, ws_bytes=big, **tab):
        t = {**ok, **tab}
        as_c = lambda v, fn: None if v is None else fn(v)
        return lib.knnsvc_harmony_f0_seg(f0, table, n, as_c(t["mask"], _i32), as_c(t["steps"], _i32), as_c(t["alpha"], _f64),
                                         as_c(t["log_ref"], _f64), out, notes, ws, ws_bytes, None)

    def refused(say, **kw):
        rc = call(**kw)
        msg = lib.knnsvc_last_error()
        assert rc != 0 and b"harmony_f0_seg" in msg and say in msg, (kw, rc, msg)

    refused(b"segment table", table=None)
    for bad, n in (((ctypes.c_int64 * 3)(0, 4, 4), 2), ((ctypes.c_int64 * 2)(1, 4), 1), (_table([2] * 65), 65), (seg, 0)):
        rc = lib.knnsvc_harmony_f0_seg(d, bad, n, _i32([1] * max(n, 1)), _i32([1] * max(n, 1)), _f64([1.0] * max(n, 1)),
                                       _f64([lr] * max(n, 1)), e, None, d, big, None)
        assert rc != 0 and b"harmony_f0_seg" in lib.knnsvc_last_error(), (n, lib.knnsvc_last_error())
    for name in ("mask", "steps", "alpha", "log_ref"):
        refused(b"null", **{name: None})
    for m in (-1, 0x1000, 1 << 20):
        refused(b"segment 1: mask", mask=[1, m])
    for v in (-25, 25, 1 << 20):
        refused(b"segment 0: steps", steps=[v, 0])
    for v in (0.0, -0.5, 1.5, float("nan"), float("inf")):
        refused(b"segment 1: alpha", alpha=[0.25, v])              # checked on an off segment too
    for v in (float("nan"), float("inf"), -float("inf")):
        refused(b"segment 0: log_ref", log_ref=[v, lr])
    refused(b"null", f0=None)
    refused(b"null", out=None)
    refused(b"null", ws=None)
    refused(b"must not be the input", out=d)
    refused(b"aligned", ws=d + 4)
    need = lib.knnsvc_tune_f0_workspace_bytes(7, 2)
    rc = call(ws_bytes=need - 1)
    assert rc == 2 and b"harmony_f0_seg: workspace" in lib.knnsvc_last_error()      # KNNSVC_EWORKSPACE


def test_mix_waves_refuses_bad_arguments_before_launching():
    lib = _lib()
    ptrs = lambda v: (ctypes.c_void_p * len(v))(*v)

    def refused(say, ys, gains, n=100, out=4096, nv=None):
        rc = lib.knnsvc_mix_waves(None if ys is None else ptrs(ys), len(gains) if nv is None else nv, None if gains is None else _f64(gains),
                                  n, out, None)
        msg = lib.knnsvc_last_error()
        assert rc == 1 and b"mix_waves" in msg and say in msg, (rc, msg)

    a, b = 1 << 16, 1 << 17
    refused(b"n_voices", [a], [1.0], nv=0)
    refused(b"n_voices", [a] * 5, [1.0] * 5)
    refused(b"null", None, [1.0], nv=1)
    refused(b"null", [a], None, nv=1)
    refused(b"null", [a], [1.0], out=None)
    refused(b"voice 1", [a, None], [1.0, 1.0])
    refused(b"length", [a], [1.0], n=-1)
    for g in (-0.5, float("nan"), float("inf")):
        refused(b"gain 1", [a, b], [1.0, g])
    refused(b"positive", [a, b], [0.0, 0.0])
    refused(b"overlaps voice 0", [a, b], [1.0, 1.0], out=a + 8)
    assert lib.knnsvc_mix_waves(ptrs([a]), 1, _f64([1.0]), 0, None, None) == 0       # nothing to do: no launch


def test_header_constants_table_and_ops_agree():
    import re
    from knn_svc_amd import _lib as L, ops, options
    src = open(os.path.join(ROOT, "include", "knnsvc_hip.h")).read()
    const = lambda name: int(re.search(rf"#define {name}\s+(\d+)", src).group(1))
    assert const("KNNSVC_HARMONY_MAX_PARTS") == ops.HARMONY_MAX_PARTS == options.HARMONY_MAX_PARTS == 3
    assert const("KNNSVC_HARMONY_MAX_STEPS") == options.HARMONY_MAX_STEPS == HO.MAX_STEPS == 24
    assert "Harmony voice" in src and L.ABI_VERSION == const("KNNSVC_ABI_VERSION")
    assert L.SIGNATURES["knnsvc_harmony_f0_seg"] == L.SIGNATURES["knnsvc_tune_f0_seg"] and len(L.SIGNATURES["knnsvc_mix_waves"][1]) == 6


def test_ops_refuse_cpu_tensors_and_all_off_returns_the_input():
    from knn_svc_amd import ops
    from knn_svc_amd.options import Harmony
    f0 = torch.full((10,), 220.0)
    sh = Harmony((2,), scale="C:major").shifts()[0]
    assert ops.harmony_f0_seg(f0, [0, 4, 10], [None, None]) is f0 and ops.harmony_f0_seg(f0, [0, 10], [None], return_notes=True) == (f0, None)
    with pytest.raises(ops.KnnSvcError, match="GPU tensor"):
        ops.harmony_f0_seg(f0, [0, 10], [sh])
    with pytest.raises(ops.KnnSvcError, match="parts for"):
        ops.harmony_f0_seg(f0, [0, 10], [sh, sh])
    with pytest.raises(ops.KnnSvcError, match="GPU tensor"):
        ops.mix_waves([f0, f0], [1.0, 0.5])
    for ys in ([], [f0] * 5):
        with pytest.raises(ops.KnnSvcError, match="voices"):
            ops.mix_waves(ys, [1.0] * len(ys))


# ---------------------------------------------------------------- entry points and the command line
def test_entry_points_refuse_before_a_file_is_read(tmp_path):
    from knn_svc_amd import matching as M, serving
    from knn_svc_amd.matcher import KNeighborsVC
    from knn_svc_amd.options import Harmony
    vc = KNeighborsVC.__new__(KNeighborsVC)                 # no models: nothing below may get as far as using one
    vc.device = torch.device("cpu")
    absent = str(tmp_path / "absent.wav")
    keyed, bare = Harmony((2, -3), scale="A:minor"), Harmony((2,))
    for bad in (2, "C:major", True, [keyed], bare):         # (bare: neither it nor a tune names a scale)
        with pytest.raises(ValueError):
            vc.special_match(absent, absent, harmony=bad)
        with pytest.raises(ValueError):
            vc.many_to_one([absent], absent, harmony=bad if not isinstance(bad, list) else [keyed, keyed])
        with pytest.raises(ValueError):
            serving.BatchConverter(vc, None, harmony=bad).convert([absent])
    for bad in (2, "C:major", keyed, [keyed.shifts()[0]] * 2):       # the match stage takes the part's shift record, one per item
        with pytest.raises(ValueError):
            M.match_features_many([torch.zeros(2, 4)], [torch.zeros(2)], None, None, None, "mix", "no_post_opt", harmony=bad)
        with pytest.raises(ValueError):
            M.match_features_blend([torch.zeros(2, 4)], [torch.zeros(2)], [None, None], None, "mix", "no_post_opt", harmony=bad)
    with pytest.raises(ValueError):
        M.match_features(None, None, None, None, None, "mix", "no_post_opt", harmony=keyed)
    conv = serving.BatchConverter(vc, None, harmony=keyed, tune="G:major")
    assert conv.harmony is keyed and conv.harmony_of(None, conv.tune) == (keyed, keyed.shifts()) and conv.harmony_of("off", None) is None
    got = conv.harmony_of([None, "off", bare], conv.tune_of([None, None, "C:major"], 3), 3)
    assert got[0] == (keyed, keyed.shifts()) and got[1] is None and got[2] == (bare, Harmony((2,), scale="C:major").shifts())
    for bad in (3, [keyed, keyed], ["x"]):
        with pytest.raises(ValueError):
            conv.convert([absent], harmony=bad)
    with pytest.raises(ValueError, match="scale"):
        serving.BatchConverter(vc, None).convert([absent], harmony=bare)
    with pytest.raises(ValueError, match="scale"):
        serving.BatchConverter(vc, None, tune="C:major").convert([absent], harmony=bare, tune="off")
    # the entry points that return one feature set per source do not take it
    import inspect
    for fn in (vc.bulk_match, M.match_at_inference_time, vc.vocode):
        assert "harmony" not in inspect.signature(fn).parameters
    for fn in (vc.special_match, vc.many_to_one, conv.convert, conv.convert_files, serving.RequestQueue.submit, M.match_features,
               M.match_features_many, M.match_features_blend):
        assert inspect.signature(fn).parameters["harmony"].default is None
    assert inspect.signature(conv.convert).parameters["stems"].default is False


def test_command_line_flags(tmp_path, capsys):
    from knn_svc_amd import inference
    from knn_svc_amd.options import Harmony, HarmonyPart
    ap = inference.build_parser()
    a = ap.parse_args(["s", "t"])
    assert (a.harmony_steps, a.harmony_scale, a.harmony_gain_db, a.harmony_lead_db, a.harmony_glide_ms) == (None,) * 5
    assert inference.harmony_of_flags(a) is None
    a = ap.parse_args(["s", "t", "--harmony_steps", "2,-3", "--harmony_scale", "A:minor", "--harmony_gain_db", "-6,-9", "--harmony_lead_db", "-1",
                       "--harmony_glide_ms", "0"])
    assert inference.harmony_of_flags(a) == Harmony((HarmonyPart(2, -6.0), HarmonyPart(-3, -9.0)), "A:minor", -1.0, 0.0)
    a = ap.parse_args(["s", "t", "--harmony_steps", "2", "--tune", "G:major"])
    assert inference.harmony_of_flags(a, inference.tuning_of(a)) == Harmony((2,))
    absent = str(tmp_path / "absent.wav")
    for bad in (["--harmony_steps", "2"],                                             # no scale, its own or --tune's
                ["--harmony_scale", "C:major"], ["--harmony_gain_db", "-6"], ["--harmony_lead_db", "0"], ["--harmony_glide_ms", "40"],
                ["--harmony_steps", "0", "--harmony_scale", "C:major"], ["--harmony_steps", "1,2,3,4", "--harmony_scale", "C:major"],
                ["--harmony_steps", "2,3", "--harmony_scale", "C:major", "--harmony_gain_db", "-6"],
                ["--harmony_steps", "2", "--harmony_scale", "H:major"], ["--harmony_steps", "2.5", "--harmony_scale", "C:major"],
                ["--harmony_steps", "2", "--harmony_scale", "C:major", "--harmony_glide_ms", "-1"]):
        with pytest.raises(SystemExit) as e:
            inference.main([absent, absent] + bad)                                    # refused before the models are loaded
        assert e.value.code == 2, bad
    with pytest.raises(SystemExit) as e:                                              # dataset mode refuses the flags
        inference.main([str(tmp_path), str(tmp_path), "--harmony_steps", "2", "--harmony_scale", "C:major"])
    assert e.value.code == 2 and "single conversion" in capsys.readouterr().err


# ---------------------------------------------------------------- the defaults call the match functions as before
def test_match_bodies_hand_harmony_on_only_when_an_item_is_a_part():
    import types
    from knn_svc_amd import matching as M
    from knn_svc_amd.options import Harmony, SourceKnobs
    sh = Harmony((2,), scale="C:major").shifts()[0]
    calls = []
    voice = types.SimpleNamespace(feats=torch.zeros(3, 4), f0=torch.zeros(3), harm=torch.zeros(3, 49))
    parts = {0: None, 1: sh, 2: None}
    saved = M.match_features, M.match_features_many, M.match_features_blend
    q = lambda i: (torch.zeros(2, 4), torch.zeros(2))
    try:
        M.match_features = lambda *a, **kw: calls.append(("one", sorted(kw), kw.get("harmony", "absent"))) or (None, None, None)
        M.match_features_many = lambda *a, **kw: calls.append(("many", sorted(kw), kw.get("harmony", "absent"))) or [(None, None, None)] * len(a[0])
        M.match_features_blend = lambda *a, **kw: calls.append(("blend", sorted(kw), kw.get("harmony", "absent"))) or [(None, None, None)] * len(a[0])
        plain = M.match_bodies(q, [voice], "mix", "no_post_opt", [({}, {})], [], lambda i: SourceKnobs())
        plain[0](0); plain[1]([0, 1])
        body, body_many = M.match_bodies(q, [voice], "mix", "no_post_opt", [({}, {})], [], lambda i: SourceKnobs(), parts=parts.__getitem__)
        body(0); body(1); body_many([0, 2]); body_many([0, 1, 2])
        blend = M.match_bodies(q, [voice, voice], "mix", "no_post_opt", [({}, {}), ({}, {})], [], lambda i: SourceKnobs(blend=(0.5, 0.5)),
                               parts=parts.__getitem__)
        blend[1]([0, 2]); blend[1]([1, 2])
    finally:
        M.match_features, M.match_features_many, M.match_features_blend = saved
    one = ["f0_shift", "nan_flags", "nn32", "pool_prep", "synth_list", "topk", "transpose"]
    many = ["f0_shift", "nan_flags", "nn32s", "pool_prep", "synth_list", "topk", "transpose"]
    blnd = ["f0_shift", "nan_flags", "nn32s", "topk", "transpose"]
    assert calls == [("one", one, "absent"), ("many", many, "absent"),
                     ("one", one, "absent"), ("one", sorted(one + ["harmony"]), sh), ("many", many, "absent"),
                     ("many", sorted(many + ["harmony"]), [None, sh, None]),
                     ("blend", blnd, "absent"), ("blend", sorted(blnd + ["harmony"]), [sh, None])]


def test_converter_without_a_harmony_builds_the_items_and_calls_of_before(monkeypatch):
    """serving.BatchConverter.convert with stand-ins for the encoder, the search, the match functions and the tail: without a
    harmony one item per source, searched and matched as before and through the whole tail; with one, the source's parts are
    further items that reuse the lead's neighbour list, run the per-voice half only, and are mixed before the per-output half."""
    import types
    from knn_svc_amd import matching as M, ops, serving
    from knn_svc_amd.options import Harmony
    log = []
    vc = types.SimpleNamespace(device=torch.device("cpu"), weighting=None, hop_length=320, sr=16000,
                               wavlm=types.SimpleNamespace(set_layer_mix=lambda m: None, n_layers=2,
                                                           encode_many=lambda ws, **kw: log.append(("encode", len(ws))) or [torch.full((3, 4), float(i)) for i in range(len(ws))]),
                               _check_finite=lambda peak: None)
    voice = types.SimpleNamespace(feats=torch.zeros(5, 4), f0=torch.zeros(5), harm=torch.zeros(5, 49), prep=None)
    monkeypatch.setattr(M, "_mix_of", lambda w, enc: None)

    def grouped(items, qpool, feats, prep, flags):
        log.append(("search", list(items)))
        return {i: torch.full((3, 1), float(i)) for i in items}, {}
    monkeypatch.setattr(M, "grouped_knn", grouped)
    monkeypatch.setattr(M, "wait_for_neighbours", lambda *a: None)

    def match_features(q, f0, *a, nn32=None, harmony="absent", **kw):
        log.append(("match", float(q[0, 0]), None if nn32 is None else float(nn32[0, 0]), harmony))
        return q, None, f0
    monkeypatch.setattr(M, "match_features", match_features)
    monkeypatch.setattr(serving.Tail, "per_voice", lambda self, of, f0, harm, src_wav=None: log.append(("voice", float(of[0, 0]))) or torch.ones(6) * (1 + float(of[0, 0])))
    monkeypatch.setattr(serving.Tail, "per_output", lambda self, y: log.append(("output", float(y[0]))) or y)
    monkeypatch.setattr(ops, "mix_waves", lambda ys, gains: log.append(("mix", len(ys), tuple(gains))) or sum(g * y for g, y in zip(ys, gains)))
    conv = serving.BatchConverter(vc, voice, match="lanes")
    srcs = [(np.zeros(960, np.float32), np.zeros(3, np.float32))] * 2
    conv.convert(srcs)
    assert log == [("encode", 2), ("search", [0, 1]), ("match", 0.0, 0.0, "absent"), ("voice", 0.0), ("output", 1.0),
                   ("match", 1.0, 1.0, "absent"), ("voice", 1.0), ("output", 2.0)]
    del log[:]
    h = Harmony((2, -3), scale="C:major", lead_db=0.0)
    out = conv.convert(srcs, harmony=[None, h], stems=False)
    s2, s3 = h.shifts()
    assert log == [("encode", 2), ("search", [0, 1]), ("match", 0.0, 0.0, "absent"), ("voice", 0.0), ("output", 1.0),
                   ("match", 1.0, 1.0, "absent"), ("voice", 1.0), ("match", 1.0, 1.0, s2), ("voice", 1.0), ("match", 1.0, 1.0, s3), ("voice", 1.0),
                   ("mix", 3, h.gains), ("output", pytest.approx(2.0 * sum(h.gains), rel=1e-6))]
    assert len(out) == 2 and float(out[0][0]) == 1.0
    del log[:]
    st = conv.convert(srcs[:1], harmony=h, stems=True)
    assert [len(s) for s in st] == [4] and ("search", [0]) in log and sum(1 for e in log if e[0] == "search") == 1
    assert [e for e in log if e[0] == "match"] == [("match", 0.0, 0.0, "absent"), ("match", 0.0, 0.0, s2), ("match", 0.0, 0.0, s3)]
