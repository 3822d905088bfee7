"""CPU: target_duration without a GPU — the oracle (tests/duration_oracle.py) against torch.nn.functional.interpolate called the
way upstream calls it, matching.duration_plan / resolve_target_duration / stretch_queries, the f0 rule, the command line, the
entry points' refusals before a file is read, and the host side of knnsvc_time_scale_seg (every argument is checked before the
launch, so dummy pointers are never dereferenced)."""
import ctypes
import dataclasses

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import duration_oracle as O

# (T, target_duration): upstream's arithmetic gives s = 15/7, 1.37, 1, 2.5, 2.5, 4, 0.25, 1.25, 0.8
CASES = [(7, 0.3), (50, 1.37), (33, 0.66), (1, 0.05), (2, 0.1), (100, 8.0), (100, 0.5), (1500, 37.5), (1500, 24.0)]


# ---------------------------------------------------------------- the oracle against F.interpolate
@pytest.mark.parametrize("T,dur", CASES)
def test_oracle_features_equal_torch_interpolate_in_fp64(T, dur):
    """Shapes equal (T_out is torch's); values within 64 * 2^-52 * max|x|.  Measured against torch 2.10 (CPU): at most
    4.5e-16 on the nine cases.  That holds because the specification forms the source index with ONE rounding (a fused
    multiply-add), as torch's CPU kernel does on a machine with FMA; with the index in two roundings the same restatement is
    1.207e-13 from torch at (1500, 37.5) against a bound of 6.018e-14 (the next test has the rows where the two differ)."""
    from knn_svc_amd import matching as M
    x = torch.from_numpy(np.random.default_rng(T).standard_normal((T, 24)))          # fp64
    target_samples = int(dur * 16000)
    s = (target_samples / 320) / x.shape[0]
    want = F.interpolate(x.T[None], scale_factor=s, mode="linear")[0].T              # upstream's call (ddsp_matcher.py:548)
    T_out, c = M.duration_plan(T, dur)
    assert (T_out, c) == O.duration_plan(T, dur) and c == 1.0 / s
    got = O.features(x.numpy(), T_out, c)
    assert got.shape == tuple(want.shape) and got.dtype == np.float64
    err = float(np.abs(got - want.numpy()).max())
    print(f"T {T} -> {T_out} (s = {s!r}): max |oracle - torch| = {err:.3e}")
    assert err <= 64 * 2.0 ** -52 * float(x.abs().max())


def test_the_fused_index_differs_from_two_roundings_only_just_above_a_power_of_two():
    """Why the index is a fused multiply-add: c * (j + 0.5) just above a power of two, r below it, and the product has been
    rounded at twice r's ulp.  At s = 1.25 that is 5 of 1875 rows, the largest difference 5.7e-14 at r ~ 512."""
    c, n = 1.0 / 1.25, 1875
    fused = O.fma_index(c, n)
    two = np.float64(c) * (np.arange(n, dtype=np.float64) + 0.5) - 0.5
    rows = np.nonzero(fused != two)[0]
    assert rows.tolist() == [1, 20, 40, 320, 640]
    assert abs(float(two[640] - fused[640])) == 2.0 ** -44 and float(np.abs(two - fused).max()) == 2.0 ** -44
    assert np.array_equal(O.fma_index(1.0, 300), np.arange(300, dtype=np.float64))        # c = 1: exact either way
    assert np.array_equal(O.fma_index(2.0, 5), [0.5, 2.5, 4.5, 6.5, 8.5])


def test_the_listed_cases_cover_both_bounds_and_the_identity():
    s = [1.0 / O.duration_plan(T, d)[1] for T, d in CASES]
    assert s[2] == 1.0 and s[5] == 4.0 and s[6] == 0.25 and s[7] == 1.25 and s[8] == 0.8
    assert O.duration_plan(1, 0.05)[0] == 2 and O.duration_plan(2, 0.1)[0] == 5


# ---------------------------------------------------------------- duration_plan / resolve_target_duration
def test_duration_plan_refuses_a_ratio_outside_the_bounds_and_an_empty_result():
    from knn_svc_amd import matching as M
    assert M.duration_plan(100, 8.0) == (400, 0.25) and M.duration_plan(100, 0.5) == (25, 4.0)
    assert M.duration_plan(100, 2.0) == (100, 1.0)
    for T, d in ((100, 8.02), (100, 0.48), (1500, 7.48), (1500, 120.02), (1, 0.01), (3, 0.019), (400, 1.98)):
        with pytest.raises(ValueError) as e:
            M.duration_plan(T, d, item="clip.wav")
        assert "clip.wav" in str(e.value)
    with pytest.raises(ValueError):        # T_out < 1 (fewer samples than one hop), whatever the ratio's bound says
        M.duration_plan(1, 0.019)
    assert (M.DURATION_SCALE_MIN, M.DURATION_SCALE_MAX) == (O.SCALE_MIN, O.SCALE_MAX) == (0.25, 4.0)


def test_resolve_target_duration_values():
    from knn_svc_amd import matching as M
    assert M.resolve_target_duration(None) is None and M.resolve_target_duration(2) == 2.0
    assert M.resolve_target_duration(np.float32(1.5)) == 1.5
    assert M.resolve_target_duration(None, 3) == [None] * 3 and M.resolve_target_duration(2.5, 2) == [2.5, 2.5]
    assert M.resolve_target_duration([None, 1, 2.5], 3) == [None, 1.0, 2.5]
    assert M.resolve_target_duration((), 0) == []


@pytest.mark.parametrize("v", [0, -1, 0.0, float("nan"), float("inf"), -float("inf"), True, False, "2", [2.0], (2.0,), {}])
def test_resolve_target_duration_refuses(v):
    from knn_svc_amd import matching as M
    with pytest.raises(ValueError):
        M.resolve_target_duration(v)


def test_resolve_target_duration_refuses_lists_of_the_wrong_length_and_bad_entries():
    from knn_svc_amd import matching as M
    for v in ([1.0, 2.0], [1.0] * 4, [1.0, None, 0], [1.0, None, True], [1.0, "2", None], [[1.0], None, None]):
        with pytest.raises(ValueError):
            M.resolve_target_duration(v, 3)


# ---------------------------------------------------------------- the f0 rule
def test_f0_tie_goes_left():
    f = np.array([100.0, 0.0, 0.0, 200.0, 300.0, 0.0], np.float32)
    i0, i1, l0, l1 = O.taps(6, 3, 2.0)                 # c = 2: r = 2j + 0.5, every l1 is exactly 0.5
    assert np.array_equal(l1, [0.5] * 3) and np.array_equal(i0, [0, 2, 4]) and np.array_equal(i1, [1, 3, 5])
    out = O.f0(f, 3, 2.0)
    assert out[0] == 100.0            # voiced | unvoiced at a tie: the left frame, unchanged
    assert out[1] == 0.0              # unvoiced | voiced at a tie: the left frame decides, unvoiced
    assert out[2] == 300.0            # voiced | unvoiced
    both = O.f0(np.array([100.0, 400.0], np.float32), 1, 2.0)
    assert abs(float(both[0]) - 200.0) < 1e-4          # two voiced neighbours: the geometric mean


def test_an_edge_never_glides_towards_zero():
    f = O.track(700, 180.0, 3)
    lo = f[f > 0].min()
    assert 0 < (f > 0).sum() < len(f)
    for s in (0.25, 0.73, 1.37, 2.5, 4.0):
        T_out, c = O.plan_for_scale(len(f), s)
        out = O.f0(f, T_out, c)
        assert out.dtype == np.float32 and out.shape == (T_out,)
        v = out[out != 0]
        assert (out >= 0).all() and v.min() >= np.nextafter(lo, np.float32(0)) and v.max() <= np.nextafter(f.max(), np.float32(1e9))
        i0, i1, l0, l1 = O.taps(len(f), T_out, c)
        near = np.where(l1 > 0.5, f[i1], f[i0])
        assert np.array_equal(out > 0, near > 0)       # voicing follows the nearer frame
        edge = (f[i0] > 0) != (f[i1] > 0)
        assert edge.any() and np.array_equal(out[edge], near[edge])      # at an edge: the nearer frame's value, bit for bit


def test_scale_one_is_the_identity():
    f = O.track(301, 220.0, 4)
    x = O.feats(301, 12, 5)
    assert np.array_equal(O.f0(f, 301, 1.0).view(np.uint32), f.view(np.uint32))
    assert np.array_equal(O.features32(x, 301, 1.0).view(np.uint32), x.view(np.uint32))
    i0, i1, l0, l1 = O.taps(301, 301, 1.0)
    assert np.array_equal(i0, np.arange(301)) and not l1.any()


def test_taps_stay_inside_the_segment():
    for T, s in ((1, 2.5), (2, 0.5), (2, 4.0), (8, 0.25), (300, 1.37), (300, 0.73), (5, 1.0)):
        T_out, c = O.plan_for_scale(T, s)
        i0, i1, l0, l1 = O.taps(T, T_out, c)
        assert T_out >= 1 and i0.min() >= 0 and i1.max() <= T - 1 and (i1 - i0).max() <= 1
        assert l1.min() >= 0 and l1.max() < 1 and np.array_equal(l0, 1.0 - l1)


# ---------------------------------------------------------------- stretch_queries
def test_stretch_queries_without_a_duration_returns_the_same_objects_and_launches_nothing(monkeypatch):
    from knn_svc_amd import matching as M, ops
    calls = []
    monkeypatch.setattr(ops, "time_scale_seg", lambda *a, **k: calls.append(a))
    feats, f0s = [torch.zeros(5, 4), torch.zeros(7, 4)], [torch.zeros(5), torch.zeros(7)]
    got_f, got_0 = M.stretch_queries(feats, f0s, [None, None])
    assert got_f is feats and got_0 is f0s and calls == []
    assert all(a is b for a, b in zip(got_f, feats))


def test_stretch_queries_makes_one_call_for_the_items_that_have_a_duration(monkeypatch):
    from knn_svc_amd import matching as M, ops
    calls = []

    def stub(x, f0, seg, out_frames, inv_scales):
        calls.append((tuple(x.shape), tuple(f0.shape), list(seg), list(out_frames), list(inv_scales)))
        n = sum(out_frames)
        return torch.arange(n * x.shape[1], dtype=torch.float32).reshape(n, -1), torch.arange(n, dtype=torch.float32)
    monkeypatch.setattr(ops, "time_scale_seg", stub)
    feats = [torch.zeros(50, 4), torch.ones(100, 4), torch.zeros(100, 4), torch.ones(20, 4)]
    f0s = [torch.zeros(50), torch.ones(100), torch.zeros(100), torch.ones(20)]
    got_f, got_0 = M.stretch_queries(feats, f0s, [None, 8.0, 0.5, None])
    assert calls == [((200, 4), (200,), [0, 100, 200], [400, 25], [0.25, 4.0])]
    assert got_f[0] is feats[0] and got_f[3] is feats[3] and got_0[0] is f0s[0] and got_0[3] is f0s[3]
    assert [t.shape[0] for t in got_f] == [50, 400, 25, 20] == [t.shape[0] for t in got_0]
    assert float(got_0[2][0]) == 400.0 and float(got_f[2][0, 0]) == 1600.0        # views of the stacked outputs, in order
    with pytest.raises(ValueError):
        M.stretch_queries(feats, f0s, [None, 8.1, None, None])
    assert len(calls) == 1


# ---------------------------------------------------------------- the record, the command line, the entry points
def test_extensions_record_is_unchanged_and_the_cli_default_is_none():
    from knn_svc_amd.inference import build_parser
    from knn_svc_amd.options import Extensions
    assert [f.name for f in dataclasses.fields(Extensions)] == ["topk", "vad_level", "f0_shift", "transpose", "loudness_db",
                                                                "envelope_mix", "peak_db"]
    ap = build_parser()
    assert ap.parse_args(["s", "t"]).target_duration is None
    a = ap.parse_args(["s", "t", "--target_duration", "12.5"])
    assert a.target_duration == 12.5 and isinstance(a.target_duration, float)


def test_main_refuses_before_loading_anything(tmp_path):
    from knn_svc_amd import inference
    absent = [str(tmp_path / "absent.wav"), str(tmp_path / "absent2.wav")]
    for extra in (["--target_duration", "0"], ["--target_duration", "-3"], ["--target_duration", "nan"],
                  ["--target_duration", "2", "--envelope_mix", "0.5"]):
        with pytest.raises(SystemExit) as e:
            inference.main(absent + extra)
        assert e.value.code == 2
    (tmp_path / "A").mkdir(); (tmp_path / "B").mkdir()
    with pytest.raises(SystemExit) as e:                    # dataset mode
        inference.main([str(tmp_path / "A"), str(tmp_path / "B"), "--target_duration", "2"])
    assert e.value.code == 2


def test_entry_points_refuse_before_a_file_is_read(tmp_path):
    from knn_svc_amd import matching as M, serving
    from knn_svc_amd.matcher import KNeighborsVC
    from knn_svc_amd.options import Extensions
    import inspect
    vc = KNeighborsVC.__new__(KNeighborsVC)                 # no models: nothing below may get as far as using one
    vc.device = torch.device("cpu")
    absent = str(tmp_path / "absent.wav")
    for kw in (dict(target_duration=0), dict(target_duration=float("nan")), dict(target_duration=True), dict(target_duration="2"),
               dict(target_duration=2.0, envelope_mix=0.5)):
        with pytest.raises(ValueError):
            vc.special_match(absent, absent, **kw)
        with pytest.raises(ValueError):
            vc.many_to_one([absent], absent, **kw)
        with pytest.raises(ValueError):                     # (takes the record, not the knob)
            M.match_at_inference_time(absent, absent, None, prioritize_f0=True, target_duration=kw["target_duration"],
                                      ext=Extensions.from_serving(envelope_mix=kw.get("envelope_mix")))
    with pytest.raises(ValueError):                         # dataset mode
        M.match_at_inference_time(absent, absent, None, prioritize_f0=True, src_dataset_path=absent, target_duration=2.0)
    with pytest.raises(ValueError):
        vc.many_to_one([absent, absent], absent, target_duration=[2.0])
    assert "target_duration" not in inspect.signature(vc.bulk_match).parameters
    assert "target_duration" not in inspect.signature(vc.vocode).parameters
    conv = serving.BatchConverter(vc, None)
    assert conv.duration_of() is None and conv.duration_of(2) == 2.0 and conv.duration_of([None, 3], 2) == [None, 3.0]
    for v in (0, [1.0], float("inf")):
        with pytest.raises(ValueError):
            conv.convert([absent], target_duration=v if not isinstance(v, list) else v * 2)
    mixed = serving.BatchConverter(vc, None, envelope_mix=0.3)
    assert mixed.duration_of(None, 2) == [None, None]
    with pytest.raises(ValueError):
        mixed.convert([absent], target_duration=2.0)
    q = serving.RequestQueue(conv, max_wait_ms=1.0)
    try:
        for v in (0, float("nan"), "2", [2.0]):
            with pytest.raises(ValueError):
                q.submit(absent, target_duration=v)
    finally:
        q.close()


def test_request_queue_hands_each_request_its_duration_and_refuses_a_bad_ratio_alone():
    """RequestQueue._run with a stand-in converter: requests with and without a duration share a batch, the batch call gets one
    entry per request, and a request whose ratio is out of bounds fails alone before the batch is formed."""
    from knn_svc_amd import serving

    class Conv:
        class vc:
            device = torch.device("cpu")

        def __init__(self):
            self.calls = []

        def pitch_of(self, f0_shift=None, transpose=None, n=None):
            return f0_shift, transpose

        def duration_of(self, d=None, n=None):
            return d

        def plan_duration(self, w, d, item=None):
            if d > 100:
                raise ValueError("ratio")

        def load_checked(self, s):
            return s, None

        def convert(self, sources, loaded=None, **kw):
            self.calls.append((list(sources), kw))
            return [torch.tensor([float(len(s))]) for s in sources]

    rq = serving.RequestQueue(Conv(), max_batch=4, max_wait_ms=5000.0)
    try:
        futs = [rq.submit("a", target_duration=2.0), rq.submit("bb"), rq.submit("ccc", target_duration=500.0),
                rq.submit("dddd", transpose=1, target_duration=3.0)]
        assert [float(futs[i].result(timeout=30)) for i in (0, 1, 3)] == [1.0, 2.0, 4.0]
        with pytest.raises(ValueError):
            futs[2].result(timeout=30)
    finally:
        rq.close()
    assert rq.batches == [4] and rq.isolated == 0
    assert rq.conv.calls == [(["a", "bb", "dddd"], dict(f0_shift=[None, None, None], transpose=[None, None, 1],
                                                       target_duration=[2.0, None, 3.0]))]


# ---------------------------------------------------------------- the C ABI
def _lib():
    import __graft_entry__ as g
    g.build()
    from knn_svc_amd import _lib
    return _lib.load()


def _table(lens):
    off = [0]
    for n in lens:
        off.append(off[-1] + n)
    return (ctypes.c_int64 * len(off))(*off)


def _f64(v):
    return (ctypes.c_double * len(v))(*v)


def test_time_scale_seg_refuses_bad_arguments_before_launching():
    lib = _lib()
    d = 256                      # a dummy, aligned, never dereferenced: every call below fails before the launch
    tin, tout, ok = _table([3, 4, 5]), _table([6, 2, 5]), _f64([0.5, 2.0, 1.0])

    def refused(*args, say):
        rc = lib.knnsvc_time_scale_seg(*args)
        msg = lib.knnsvc_last_error()
        assert rc != 0 and b"time_scale_seg" in msg and say in msg, (args, rc, msg)

    refused(d, 8, d, tin, tout, _f64([0.5, 0.0, 1.0]), 3, d, d, None, say=b"segment 1")
    refused(d, 8, d, tin, tout, _f64([0.5, 2.0, -1.0]), 3, d, d, None, say=b"segment 2")
    refused(d, 8, d, tin, tout, _f64([float("nan"), 2.0, 1.0]), 3, d, d, None, say=b"segment 0")
    refused(d, 8, d, tin, tout, _f64([0.5, float("inf"), 1.0]), 3, d, d, None, say=b"inv_scale")
    refused(d, 8, d, tin, tout, None, 3, d, d, None, say=b"inv_scale")
    refused(d, 8, d, tin, tout, ok, 3, None, d, None, say=b"x_out")
    refused(None, 8, d, tin, tout, ok, 3, d, d, None, say=b"x_out")
    refused(d, 8, d, tin, tout, ok, 3, d, None, None, say=b"f0_out")
    refused(d, 8, None, tin, tout, ok, 3, d, d, None, say=b"f0_out")
    refused(None, 8, None, tin, tout, ok, 3, None, None, None, say=b"nothing to do")
    refused(d, 0, None, tin, tout, ok, 3, d, None, None, say=b"dim")
    refused(d, 8, d, None, tout, ok, 3, d, d, None, say=b"segment table")
    refused(d, 8, d, tin, None, ok, 3, d, d, None, say=b"segment table")
    for bad, n in (((ctypes.c_int64 * 3)(0, 4, 4), 2), ((ctypes.c_int64 * 2)(1, 4), 1), (_table([2] * 65), 65), (tin, 0)):
        good = _table([2] * max(n, 1))
        for a, b in ((bad, good), (good, bad)):          # an empty output segment (T' = 0) is refused like an empty input one
            rc = lib.knnsvc_time_scale_seg(d, 8, d, a, b, _f64([1.0] * max(n, 1)), n, d, d, None)
            assert rc != 0 and b"time_scale_seg" in lib.knnsvc_last_error(), (n, lib.knnsvc_last_error())


def test_header_and_table_agree_on_the_new_entry():
    import os
    import re
    from knn_svc_amd import _lib as L
    lib = _lib()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = open(os.path.join(root, "include", "knnsvc_hip.h")).read()
    assert re.search(r"\bint knnsvc_time_scale_seg\(", src) and "Time scale" in src
    res, args = L.SIGNATURES["knnsvc_time_scale_seg"]
    assert len(args) == 10 and args[1] is ctypes.c_int32 and args[6] is ctypes.c_int32 and hasattr(lib, "knnsvc_time_scale_seg")
    assert "timescale.hip" in open(os.path.join(root, "knn_svc_amd", "csrc", "Makefile")).read()
    assert lib.knnsvc_abi_version() == L.ABI_VERSION


def test_ops_time_scale_refuses_cpu_tensors_and_bad_tables():
    from knn_svc_amd import ops
    with pytest.raises(ops.KnnSvcError):
        ops.time_scale_seg(torch.zeros(4, 8), torch.zeros(4), [0, 4], [5], [0.8])
    with pytest.raises(ops.KnnSvcError):
        ops.time_scale_seg(None, None, [0, 4], [5], [0.8])
    with pytest.raises(ops.KnnSvcError):
        ops.time_scale(torch.zeros(4, 8), None, 5, 0.8)
