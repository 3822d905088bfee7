"""CPU: pitch correction without a GPU — options.Tuning and its scale grammar, matching.resolve_tune, the oracle's own properties
(tests/tune_oracle.py), the C ABI of knnsvc_tune_f0_seg (every argument is checked before the launch, so dummy pointers are never
dereferenced), the command line and the entry points' refusals before a file is read, and the precondition of the GPU tests:
every f0 case the GPU child compares notes on stands at least 1e-6 semitone from every note decision going the other way."""
import ctypes
import dataclasses
import inspect
import math
import os
import re

import numpy as np
import pytest
import torch

import tune_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------- the scale grammar and the record
def test_relative_and_enharmonic_keys_give_the_same_mask():
    from knn_svc_amd.options import Tuning, scale_mask
    assert scale_mask("A:minor") == scale_mask("C:major") == 0b101010110101
    assert scale_mask("F#:major") == scale_mask("Gb:major") == scale_mask("gb:MAJOR")
    assert scale_mask("chromatic") == scale_mask("Chromatic") == 0xFFF
    assert scale_mask("E:minor") == scale_mask("G:major") and scale_mask("C:major") != scale_mask("G:major")
    assert scale_mask("A:minor_pentatonic") == scale_mask("C:pentatonic")
    assert Tuning("Bb:blues").mask == scale_mask("A#:blues")


def test_every_tonic_and_name_agrees_with_the_oracles_restatement():
    from knn_svc_amd import options
    tonics = "C C# Db D D# Eb E F F# Gb G G# Ab A A# Bb B".split()
    names = ("major", "minor", "harmonic_minor", "pentatonic", "minor_pentatonic", "blues")
    assert sorted(options.TUNE_TONICS) == sorted(t.lower() for t in tonics) and tuple(options.TUNE_SCALES) == names
    for t in tonics:
        for name in names:
            m = options.scale_mask(f"{t}:{name}")
            assert m == O.mask_of(f"{t}:{name}") and 0 < m <= 0xFFF and (m >> O.TONICS[t.lower()]) & 1      # the tonic is in its scale


def test_patterns_are_relative_to_the_tonic():
    from knn_svc_amd.options import scale_mask
    assert scale_mask("C:100000000000") == 1 and scale_mask("A:100000000000") == 1 << 9
    assert scale_mask("D:101011010101") == scale_mask("D:major")
    assert scale_mask("B:110000000000") == (1 << 11) | 1                      # wraps round to C
    assert scale_mask("G:111111111111") == 0xFFF
    assert scale_mask(O.CUSTOM) == O.mask_of(O.CUSTOM) == sum(1 << k for k in (2, 5, 7, 10, 0))


def test_tuning_defaults_and_derived_values():
    from knn_svc_amd.options import TUNE_OFF, SourceKnobs, Tuning
    t = Tuning("A:minor")
    assert (t.strength, t.retune_ms, t.tuning_hz) == (1.0, 80.0, 440.0) and t.on
    assert t.alpha == -math.expm1(-20.0 / 80.0) and t.log_ref == math.log(440.0)
    assert Tuning("chromatic", retune_ms=0).alpha == 1.0 and 0 < Tuning("chromatic", retune_ms=2000).alpha < 0.01
    assert Tuning("chromatic", strength=np.float32(0.5), tuning_hz=np.int64(442)) == Tuning("chromatic", 0.5, 80.0, 442.0)
    for t in (Tuning("C:major", 0.6, 200.0, 415.0), Tuning(O.CUSTOM, 1, 0)):
        want = O.T(t.scale, t.strength, t.retune_ms, t.tuning_hz)
        assert (t.mask, t.strength, t.alpha, t.log_ref) == tuple(want)[:4] and Tuning(*want.spec) == t
    assert not TUNE_OFF.on and not Tuning("C:major", strength=0).on
    with pytest.raises(dataclasses.FrozenInstanceError):
        t.strength = 0.5
    assert SourceKnobs().tune is None and [f.name for f in dataclasses.fields(SourceKnobs)][-1] == "tune"


@pytest.mark.parametrize("kw", [
    dict(scale="H:major"), dict(scale="C"), dict(scale="major"), dict(scale="C:maj"), dict(scale="C:10101101010"),
    dict(scale="C:1010110101012"), dict(scale="C:000000000000"), dict(scale="C:10101101010x"), dict(scale=""), dict(scale=None),
    dict(scale=0xFFF), dict(scale="Cb:major"), dict(scale="chromatic", strength=-0.1), dict(scale="chromatic", strength=1.1),
    dict(scale="chromatic", strength=float("nan")), dict(scale="chromatic", strength=True), dict(scale="chromatic", strength="1"),
    dict(scale="chromatic", strength=None), dict(scale="chromatic", retune_ms=-1), dict(scale="chromatic", retune_ms=2000.5),
    dict(scale="chromatic", retune_ms=float("inf")), dict(scale="chromatic", retune_ms=False), dict(scale="chromatic", retune_ms="80"),
    dict(scale="chromatic", tuning_hz=399.9), dict(scale="chromatic", tuning_hz=481), dict(scale="chromatic", tuning_hz=np.bool_(True)),
    dict(scale="chromatic", tuning_hz="440"), dict(scale="chromatic", tuning_hz=float("nan"))])
def test_tuning_refuses(kw):
    from knn_svc_amd.options import Tuning
    with pytest.raises(ValueError):
        Tuning(**kw)


def test_resolve_tune():
    from knn_svc_amd import matching as M
    from knn_svc_amd.options import TUNE_OFF, Tuning
    t = Tuning("G:major", 0.5)
    assert M.resolve_tune(None) is None and M.resolve_tune(t) is t and M.resolve_tune("off") is TUNE_OFF is M.resolve_tune("OFF")
    assert M.resolve_tune("A:minor") == Tuning("A:minor") and M.resolve_tune("chromatic").mask == 0xFFF
    assert M.resolve_tune(None, 3) == [None] * 3 and M.resolve_tune("C:major", 2) == [Tuning("C:major")] * 2
    assert M.resolve_tune([None, "off", "chromatic", t], 4) == [None, TUNE_OFF, Tuning("chromatic"), t]
    assert M.resolve_tune([], 0) == [] and M.resolve_tune((t,), 1) == [t]
    assert not M.tune_active([None, TUNE_OFF]) and not M.tune_active([]) and M.tune_active([None, t])
    for bad in ("H:major", "", 3, 0.5, True, {"scale": "chromatic"}, b"chromatic"):
        with pytest.raises(ValueError):
            M.resolve_tune(bad)
    for bad, n in ((["chromatic"], 2), (["chromatic", "x"], 2), ([None, 7], 2), ("nonsense", 2), ([], 1)):
        with pytest.raises(ValueError):
            M.resolve_tune(bad, n)
    with pytest.raises(ValueError):
        M.resolve_tune(["chromatic"])                        # a list where one value is expected


# ---------------------------------------------------------------- the oracle's own properties
def test_oracle_a_flat_tone_30_cents_sharp_lands_on_the_grid_of_440():
    x = O.hz(np.full(80, 60.3))
    y, notes, margin = O.tune(x, [0, 80], [O.T("chromatic", 1.0, 0.0)])
    assert (notes == 60).all() and margin > 0.3
    assert np.array_equal(y, O.grid_hz(notes).astype(np.float32)) and abs(float(y[0]) - 261.6255653) < 1e-4
    y2, n2, _ = O.tune(x, [0, 80], [O.T("chromatic", 1.0, 0.0, 442.0)])
    assert (n2 == 60).all() and np.allclose(y2, O.grid_hz(n2, 442.0), rtol=1e-7, atol=0)
    # a slow retune of a flat tone is still a full correction (g starts at e and e is constant), half strength goes half way
    y3, _, _ = O.tune(x, [0, 80], [O.T("chromatic", 1.0, 200.0)])
    assert np.array_equal(y3, y)
    y4, _, _ = O.tune(x, [0, 80], [O.T("chromatic", 0.5, 0.0)])
    assert np.allclose(np.log(y4.astype(np.float64)), 0.5 * (np.log(x.astype(np.float64)) + np.log(y.astype(np.float64))), rtol=0, atol=1e-7)


def test_oracle_nothing_looks_across_a_segment_boundary():
    a = np.concatenate([np.zeros(4, np.float32), O.hz(np.full(20, 64.3))])           # ends pitched
    b = np.concatenate([O.hz(np.full(20, 67.4)), np.zeros(3, np.float32)])           # begins pitched, 3 semitones away
    t = O.T("chromatic", 1.0, 120.0)
    y, n, _ = O.tune(np.concatenate([a, b]), [0, a.size, a.size + b.size], [t, t])
    ya, na, _ = O.tune(a, [0, a.size], [t])
    yb, nb, _ = O.tune(b, [0, b.size], [t])
    assert np.array_equal(y.view(np.uint32), np.concatenate([ya, yb]).view(np.uint32)) and np.array_equal(n, np.concatenate([na, nb]))
    assert na[-1] == 64 and nb[0] == 67
    # as ONE segment the two halves are one run: the median window and the hysteresis carry across, and the result differs
    y1, n1, _ = O.tune(np.concatenate([a, b]), [0, a.size + b.size], [t])
    assert not np.array_equal(y1, y)


def test_oracle_an_off_segment_and_unpitched_frames_keep_their_bits():
    odd = np.array([0.0, -0.0, np.nan, np.inf, -np.inf, -220.0, 220.0, 0.0, 1e-45], np.float32)
    for t in (None, O.T_(0, 1.0, 1.0, math.log(440.0)), O.T("chromatic", 0.0)):
        y, n, margin = O.tune(odd, [0, odd.size], [t])
        assert np.array_equal(y.view(np.uint32), odd.view(np.uint32)) and (n == -1).all() and margin == np.inf
    y, n, _ = O.tune(odd, [0, odd.size], [O.T("chromatic", 1.0, 0.0)])
    unp = [0, 1, 2, 3, 4, 5, 7]
    assert np.array_equal(y[unp].view(np.uint32), odd[unp].view(np.uint32)) and (n[unp] == -1).all()
    assert n[6] == 57 and abs(float(y[6]) - 220.0) < 1e-4 and n[8] < -1000 and y[8] > 0          # a denormal is pitched


def test_oracle_hysteresis_and_slow_retune_keep_vibrato():
    i = np.arange(400)
    x = O.hz(64.2 + 0.5 * np.sin(2 * np.pi * 5.5 * i * 0.02))                      # +-0.5 semitone at 5.5 Hz, 20 cents sharp
    semis = lambda y: (np.log(y.astype(np.float64)) - math.log(440.0)) / O.S + 69.0
    y, n, _ = O.tune(x, [0, 400], [O.T("chromatic", 1.0, 80.0)])
    m = semis(y)[100:]
    assert set(n.tolist()) == {64} and abs(m.mean() - 64.0) < 0.002 and 0.80 <= (m.max() - m.min()) / 2 / 0.5 <= 0.84
    y, n, _ = O.tune(x, [0, 400], [O.T("chromatic", 1.0, 200.0)])
    m = semis(y)[100:]
    assert abs(m.mean() - 64.0) < 0.002 and 0.93 <= (m.max() - m.min()) / 2 / 0.5 <= 0.95
    y, n, _ = O.tune(x, [0, 400], [O.T("chromatic", 1.0, 0.0)])
    assert np.abs(semis(y) - 64.0).max() < 1e-5                                    # a hard snap removes it


def test_oracle_near_prefers_the_lower_of_two_equally_near_notes():
    assert O.near(0xFFF, np.float64(60.5))[0] == 60 and O.near(0xFFF, np.float64(-0.5))[0] == -1
    assert O.near(1, np.float64(66.0))[0] == 60 and O.near(1, np.float64(66.0))[1:] == (6.0, 6.0)
    assert O.near(O.mask_of("C:major"), np.float64(61.2))[0] == 62 and O.near(O.mask_of("C:major"), np.float64(60.9))[0] == 60
    assert O.near(1 << 11, np.float64(-3.0))[0] == -1                             # pitch classes of negative notes


# ---------------------------------------------------------------- the precondition of the GPU tests
def test_every_gpu_kernel_case_stands_clear_of_a_decision_boundary():
    """The device's and numpy's fp64 log may differ by a few ulp, 1e-13 of m; a decision 1e-6 away cannot flip, so the GPU tests
    may compare notes exactly.  A condition on the inputs, not a measurement."""
    cases = O.kernel_cases()
    assert set(cases) == {"edges", "up", "up-shifted", "down", "down-shifted", "near", "near-shifted", "steps", "one-run"}
    for name, (f0, seg, tunings) in cases.items():
        _y, notes, margin = O.tune(f0, seg, tunings)
        assert margin >= 1e-6, (name, margin)
        assert (notes >= 0).any(), name
    assert cases["steps"][1][1] == 954 and cases["one-run"][1][1] == 1500
    assert [cases[k][1][1] for k in ("up", "down", "near")] == [1237, 777, 301]
    f0, seg, tunings, why = O.edges()
    assert tunings[8] is None and len({t.mask for t in tunings if t}) >= 6 and len({t.log_ref for t in tunings if t}) >= 4
    assert any(seg[s + 1] - seg[s] == 1 for s in range(len(seg) - 1)) and len(why) == len(tunings)


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


def _f64(v):
    return (ctypes.c_double * len(v))(*v)


def _i32(v):
    return (ctypes.c_int32 * len(v))(*v)


def test_tune_f0_seg_refuses_bad_arguments_before_launching():
    lib = _lib()
    d, e = 256, 512              # dummies, aligned, never dereferenced: every call below fails before the launch
    seg = _table([3, 4])
    lr = math.log(440.0)
    ok = dict(mask=[0xFFF, 0], sigma=[1.0, 0.0], alpha=[0.25, 1.0], log_ref=[lr, lr])
    big = 1 << 20

    def call(f0=d, table=seg, n=2, out=e, notes=None, ws=d, ws_bytes=big, **tab):
        t = {**ok, **tab}
        as_c = lambda v, fn: None if v is None else fn(v)
        return lib.knnsvc_tune_f0_seg(f0, table, n, as_c(t["mask"], _i32), as_c(t["sigma"], _f64), as_c(t["alpha"], _f64),
                                      as_c(t["log_ref"], _f64), out, notes, ws, ws_bytes, None)

    def refused(say, **kw):
        rc = call(**kw)
        msg = lib.knnsvc_last_error()
        assert rc != 0 and b"tune_f0_seg" in msg and say in msg, (kw, rc, msg)

    refused(b"segment table", table=None)
    for bad, n in (((ctypes.c_int64 * 3)(0, 4, 4), 2), ((ctypes.c_int64 * 2)(1, 4), 1), (_table([2] * 65), 65), (seg, 0)):
        rc = lib.knnsvc_tune_f0_seg(d, bad, n, _i32([1] * max(n, 1)), _f64([1.0] * max(n, 1)), _f64([1.0] * max(n, 1)),
                                    _f64([lr] * max(n, 1)), e, None, d, big, None)
        assert rc != 0 and b"tune_f0_seg" in lib.knnsvc_last_error(), (n, lib.knnsvc_last_error())
    for name in ("mask", "sigma", "alpha", "log_ref"):
        refused(b"null", **{name: None})
    for m in (-1, 0x1000, 1 << 20):
        refused(b"segment 1: mask", mask=[1, m])
    for v in (-0.1, 1.0000001, float("nan"), float("inf")):
        refused(b"segment 0: sigma", sigma=[v, 0.0])
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
    assert need >= 7 * 28
    refused(b"workspace", ws_bytes=need - 1)
    assert call(ws_bytes=need - 1) == 2                            # KNNSVC_EWORKSPACE
    for n_total, n_seg in ((0, 1), (-5, 1), (1, 2), (10, 0), (100, 65)):
        assert lib.knnsvc_tune_f0_workspace_bytes(n_total, n_seg) == 0 and b"tune_f0" in lib.knnsvc_last_error()
    assert lib.knnsvc_tune_f0_workspace_bytes(1, 1) > 0
    assert lib.knnsvc_tune_f0_workspace_bytes(2000, 3) == lib.knnsvc_tune_f0_workspace_bytes(2000, 64)


def test_header_table_and_library_agree_on_both_entries():
    from knn_svc_amd import _lib as L
    lib = _lib()
    src = open(os.path.join(ROOT, "include", "knnsvc_hip.h")).read()
    assert re.search(r"\bsize_t knnsvc_tune_f0_workspace_bytes\(int64_t n_total, int32_t n_seg\);", src)
    assert re.search(r"\bint knnsvc_tune_f0_seg\(", src) and "Pitch correction" in src
    assert re.search(r"#define KNNSVC_EWORKSPACE 2\b", src)                    # (the code asserted above)
    res, args = L.SIGNATURES["knnsvc_tune_f0_workspace_bytes"]
    assert res is ctypes.c_size_t and args == [ctypes.c_int64, ctypes.c_int32]
    res, args = L.SIGNATURES["knnsvc_tune_f0_seg"]
    assert res is ctypes.c_int32 and len(args) == 12 and args[2] is ctypes.c_int32 and args[10] is ctypes.c_size_t
    assert hasattr(lib, "knnsvc_tune_f0_seg") and hasattr(lib, "knnsvc_tune_f0_workspace_bytes")
    assert "tune.hip" in open(os.path.join(ROOT, "knn_svc_amd", "csrc", "Makefile")).read()
    assert lib.knnsvc_abi_version() == L.ABI_VERSION


# ---------------------------------------------------------------- ops, the command line, the entry points
def test_all_off_returns_the_input_object_and_never_loads_the_library(monkeypatch):
    from knn_svc_amd import _lib as L, ops
    from knn_svc_amd.options import TUNE_OFF, Tuning

    def no_load():
        raise AssertionError("the library must not be loaded when nothing is on")
    monkeypatch.setattr(L, "load", no_load)
    x = torch.tensor([220.0, 0.0, 233.0, 247.0])
    assert ops.tune_f0_seg(x, [0, 4], [None]) is x
    assert ops.tune_f0_seg(x, [0, 1, 4], [None, TUNE_OFF]) is x
    assert ops.tune_f0_seg(x, ops.Segments([0, 2, 4]), [Tuning("C:major", strength=0), None]) is x
    y, notes = ops.tune_f0_seg(x, [0, 4], [None], return_notes=True)
    assert y is x and notes is None
    with pytest.raises(ops.KnnSvcError):
        ops.tune_f0_seg(x, [0, 4], [None, None])                       # the count is checked even then
    with pytest.raises(ops.KnnSvcError):
        ops.tune_f0_seg(x, [0, 4], [Tuning("C:major")])                # on: a CPU tensor is refused (there is no CPU path)


def test_the_defaults_of_every_entry_point_mean_nothing_is_launched():
    from knn_svc_amd import matching as M, serving
    from knn_svc_amd.inference import build_parser, tuning_of
    from knn_svc_amd.matcher import KNeighborsVC
    from knn_svc_amd.options import Extensions
    par = lambda fn: inspect.signature(fn).parameters
    for fn in (KNeighborsVC.special_match, KNeighborsVC.bulk_match, KNeighborsVC.many_to_one, M.match_at_inference_time,
               M.match_features, M.match_features_many, M.match_features_blend, serving.BatchConverter.__init__,
               serving.BatchConverter.convert, serving.BatchConverter.convert_files, serving.RequestQueue.submit):
        assert par(fn)["tune"].default is None, fn
        assert not M.tune_active([M.resolve_tune(par(fn)["tune"].default)])
    assert "tune" not in par(KNeighborsVC.vocode)
    assert [f.name for f in dataclasses.fields(Extensions)] == ["topk", "vad_level", "f0_shift", "transpose", "loudness_db",
                                                                "envelope_mix", "peak_db"]
    a = build_parser().parse_args(["s", "t"])
    assert (a.tune, a.tune_strength, a.retune_ms, a.tuning_hz) == (None,) * 4 and tuning_of(a) is None
    a = build_parser().parse_args(["s", "t", "--tune", "A:minor", "--tune_strength", "0.5", "--retune_ms", "0", "--tuning_hz", "442"])
    t = tuning_of(a)
    assert (t.scale, t.strength, t.retune_ms, t.tuning_hz, t.alpha) == ("A:minor", 0.5, 0.0, 442.0, 1.0)
    vc = KNeighborsVC.__new__(KNeighborsVC)
    vc.device = torch.device("cpu")
    conv = serving.BatchConverter(vc, None)
    assert conv.tune is None and conv.tune_of() is None and conv.tune_of(None, 3) == [None] * 3


def test_main_refuses_before_loading_anything(tmp_path):
    from knn_svc_amd import inference
    absent = [str(tmp_path / "absent.wav"), str(tmp_path / "absent2.wav")]
    for extra in (["--tune_strength", "0.5"], ["--retune_ms", "40"], ["--tuning_hz", "442"],          # refinements without --tune
                  ["--tune", "H:major"], ["--tune", "C:maj"], ["--tune", "C:000000000000"], ["--tune", ""],
                  ["--tune", "chromatic", "--tune_strength", "1.5"], ["--tune", "chromatic", "--tune_strength", "nan"],
                  ["--tune", "chromatic", "--retune_ms", "-1"], ["--tune", "chromatic", "--retune_ms", "2001"],
                  ["--tune", "chromatic", "--tuning_hz", "399"], ["--tune", "chromatic", "--tuning_hz", "x"]):
        with pytest.raises(SystemExit) as e:
            inference.main(absent + extra)
        assert e.value.code == 2, extra
    (tmp_path / "A").mkdir(); (tmp_path / "B").mkdir()
    with pytest.raises(SystemExit) as e:                                                       # folder mode takes --tune; a bad one is refused
        inference.main([str(tmp_path / "A"), str(tmp_path / "B"), "--tune", "Z:minor"])
    assert e.value.code == 2


def test_entry_points_refuse_before_a_file_is_read(tmp_path):
    from knn_svc_amd import matching as M, serving
    from knn_svc_amd.matcher import KNeighborsVC
    from knn_svc_amd.options import TUNE_OFF, Tuning
    vc = KNeighborsVC.__new__(KNeighborsVC)                 # no models: nothing below may get as far as using one
    vc.device = torch.device("cpu")
    absent = str(tmp_path / "absent.wav")
    for bad in ("H:major", "C:000000000000", 3, True, ["chromatic"]):
        with pytest.raises(ValueError):
            vc.special_match(absent, absent, tune=bad)
        with pytest.raises(ValueError):
            vc.bulk_match(absent, absent, absent, tune=bad)
        with pytest.raises(ValueError):
            M.match_at_inference_time(absent, absent, None, tune=bad)
        with pytest.raises(ValueError):
            M.match_features(None, None, None, None, None, "mix", "no_post_opt", tune=bad)
        with pytest.raises(ValueError):
            serving.BatchConverter(vc, None, tune=bad)
    for bad in ("H:major", 3, ["chromatic", "C:major"], [None, "x"]):
        with pytest.raises(ValueError):
            vc.many_to_one([absent], absent, tune=bad)
        with pytest.raises(ValueError):
            M.match_features_many([torch.zeros(2, 4)], [torch.zeros(2)], None, None, None, "mix", "no_post_opt", tune=bad)
        with pytest.raises(ValueError):
            M.match_features_blend([torch.zeros(2, 4)], [torch.zeros(2)], [None, None], None, "mix", "no_post_opt", tune=bad)
    conv = serving.BatchConverter(vc, None, tune="G:major")
    g = Tuning("G:major")
    assert conv.tune == g and conv.tune_of() == g and conv.tune_of("off") is TUNE_OFF and conv.tune_of("chromatic") == Tuning("chromatic")
    assert conv.tune_of(None, 2) == [g, g] and conv.tune_of("off", 2) == [TUNE_OFF] * 2
    assert conv.tune_of([None, "off", "A:minor"], 3) == [g, TUNE_OFF, Tuning("A:minor")]
    for bad in ("H:major", ["chromatic", "chromatic"], [7], 0.5):
        with pytest.raises(ValueError):
            conv.convert([absent], tune=bad)
    q = serving.RequestQueue(conv, max_wait_ms=1.0)
    try:
        for bad in ("H:major", 3, ["chromatic"], "C:000000000000"):
            with pytest.raises(ValueError):
                q.submit(absent, tune=bad)                  # fails alone, at the door
    finally:
        q.close()


def test_request_queue_hands_each_request_its_key():
    """RequestQueue._run with a stand-in converter: requests with and without a key of their own share a batch, the batch call
    gets one entry per request (None: the converter's default), and a batch without any is converted as it always was."""
    from knn_svc_amd import serving
    from knn_svc_amd.options import Tuning

    class Conv:
        class vc:
            device = torch.device("cpu")

        def __init__(self):
            self.calls = []

        tune_of = serving.BatchConverter.tune_of
        tune = None

        def load_checked(self, s):
            return s, None

        def convert(self, sources, loaded=None, **kw):
            self.calls.append((list(sources), kw))
            return [torch.tensor([float(len(s))]) for s in sources]

    rq = serving.RequestQueue(Conv(), max_batch=3, max_wait_ms=5000.0)
    try:
        with pytest.raises(ValueError):
            rq.submit("zz", tune="H:major")
        futs = [rq.submit("a", tune="A:minor"), rq.submit("bb"), rq.submit("ccc", tune=Tuning("chromatic", 0.5))]
        assert [float(f.result(timeout=30)) for f in futs] == [1.0, 2.0, 3.0]
        futs = [rq.submit(s) for s in ("x", "yy", "zzz")]
        assert [float(f.result(timeout=30)) for f in futs] == [1.0, 2.0, 3.0]
    finally:
        rq.close()
    assert rq.batches == [3, 3] and rq.isolated == 0
    assert rq.conv.calls == [(["a", "bb", "ccc"], dict(tune=[Tuning("A:minor"), None, Tuning("chromatic", 0.5)])),
                             (["x", "yy", "zzz"], {})]


def test_match_bodies_hand_tune_on_only_when_an_item_has_one():
    """matching.match_bodies with recording stand-ins: a batch whose items carry no key calls the match functions exactly as
    before (no ``tune`` argument); a batch in which one does hands on the per-item list."""
    import types
    from knn_svc_amd import matching as M
    from knn_svc_amd.options import TUNE_OFF, SourceKnobs, Tuning
    calls = []
    voice = types.SimpleNamespace(feats=torch.zeros(3, 4), f0=torch.zeros(3), harm=torch.zeros(3, 49))
    knobs = {0: SourceKnobs(), 1: SourceKnobs(tune=Tuning("C:major")), 2: SourceKnobs(tune=TUNE_OFF)}
    saved = M.match_features, M.match_features_many
    try:
        M.match_features = lambda *a, **kw: calls.append(("one", kw.get("tune", "absent"))) or (None, None, None)
        M.match_features_many = lambda *a, **kw: calls.append(("many", kw.get("tune", "absent"))) or [(None, None, None)] * len(a[0])
        body, body_many = M.match_bodies(lambda i: (torch.zeros(2, 4), torch.zeros(2)), [voice], "mix", "no_post_opt", [({}, {})], [],
                                         knobs.__getitem__)
        body(0); body(2); body(1); body_many([0, 2]); body_many([0, 1, 2])
    finally:
        M.match_features, M.match_features_many = saved
    assert calls == [("one", "absent"), ("one", "absent"), ("one", Tuning("C:major")), ("many", "absent"),
                     ("many", [None, Tuning("C:major"), TUNE_OFF])]
