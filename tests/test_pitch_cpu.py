"""CPU: pitch control (f0_shift / transpose) without a GPU — the command line, matching.resolve_f0_shift, the host side of
knnsvc_shift_f0_seg_mode (every argument is checked before the launch, so dummy pointers are never dereferenced), and the
oracle's own properties on the f0 cases the GPU tests use (tests/pitch_oracle.py)."""
import ctypes

import numpy as np
import pytest

import pitch_oracle as O


# ---------------------------------------------------------------- command line
def test_parser_has_the_flags_with_upstream_defaults():
    from knn_svc_amd.inference import build_parser
    ap = build_parser()
    a = ap.parse_args(["s", "t"])
    assert a.f0_shift == "median" and a.transpose == 0 and isinstance(a.transpose, float)
    a = ap.parse_args(["s", "t", "--f0_shift", "semitone", "--transpose", "-2.5"])
    assert (a.f0_shift, a.transpose) == ("semitone", -2.5)
    for m in ("median", "octave", "semitone", "none"):
        assert ap.parse_args(["s", "t", "--f0_shift", m]).f0_shift == m
    with pytest.raises(SystemExit):
        ap.parse_args(["s", "t", "--f0_shift", "fifth"])


def test_main_refuses_a_transpose_out_of_range_before_loading_anything(tmp_path):
    from knn_svc_amd import inference
    with pytest.raises(SystemExit) as e:
        inference.main([str(tmp_path / "absent.wav"), str(tmp_path / "absent2.wav"), "--transpose", "40"])
    assert e.value.code == 2


# ---------------------------------------------------------------- resolve_f0_shift
def test_resolve_f0_shift_values():
    from knn_svc_amd import matching as M
    assert M.F0_SHIFT_MODES == {"median": 0, "octave": 1, "semitone": 2, "none": 3} == O.MODES
    assert M.resolve_f0_shift(None, None) == (0, 0.0)
    assert M.resolve_f0_shift("octave", 3) == (1, 3.0)
    assert M.resolve_f0_shift("none", -36) == (3, -36.0) and M.resolve_f0_shift("semitone", 36.0) == (2, 36.0)
    assert M.resolve_f0_shift("median", np.float32(0.5)) == (0, 0.5)
    assert M.resolve_f0_shift("octave", 0.0, 3) == ([1, 1, 1], [0.0, 0.0, 0.0])
    assert M.resolve_f0_shift(["median", "none", None], [1, None, -2.0], 3) == ([0, 3, 0], [1.0, 0.0, -2.0])
    assert M.resolve_f0_shift("none", [0, 12], 2) == ([3, 3], [0.0, 12.0])


@pytest.mark.parametrize("mode,t", [("fifth", 0), ("Median", 0), (4, 0), (0, 0), (True, 0), ("median", float("nan")),
                                    ("median", float("inf")), ("none", -float("inf")), ("octave", 36.5), ("octave", -37),
                                    ("semitone", True), ("semitone", False), ("none", "2"), ("none", [1.0])])
def test_resolve_f0_shift_refuses(mode, t):
    from knn_svc_amd import matching as M
    with pytest.raises(ValueError):
        M.resolve_f0_shift(mode, t)


def test_resolve_f0_shift_refuses_lists_of_the_wrong_length_and_bad_entries():
    from knn_svc_amd import matching as M
    for mode, t in ((["median", "none"], 0), ("median", [0.0, 1.0, 2.0, 3.0]), (["median"] * 3, [0.0] * 2),
                    (["median", "none", "fifth"], 0), ("median", [0.0, float("nan"), 0.0]), ("median", [0.0, 1.0, True])):
        with pytest.raises(ValueError):
            M.resolve_f0_shift(mode, t, 3)


def test_entry_points_refuse_bad_values_before_a_file_is_read(tmp_path):
    """special_match / bulk_match / many_to_one / match_at_inference_time / BatchConverter / RequestQueue.submit: the value is
    checked first, so paths that do not exist are never opened and no model is needed."""
    from knn_svc_amd import matching as M, serving
    from knn_svc_amd.matcher import KNeighborsVC
    import torch
    vc = KNeighborsVC.__new__(KNeighborsVC)                 # no models: nothing below may get as far as using one
    vc.device = torch.device("cpu")
    absent = str(tmp_path / "absent.wav")
    for kw in (dict(f0_shift="fifth"), dict(transpose=float("nan")), dict(transpose=36.5), dict(transpose=True)):
        with pytest.raises(ValueError):
            vc.special_match(absent, absent, **kw)
        with pytest.raises(ValueError):
            vc.bulk_match(absent, absent, absent, **kw)
        with pytest.raises(ValueError):
            vc.many_to_one([absent], absent, **kw)
        with pytest.raises(ValueError):
            M.match_at_inference_time(absent, absent, None, prioritize_f0=True, **kw)
        with pytest.raises(ValueError):
            serving.BatchConverter(vc, None, **kw)
    conv = serving.BatchConverter(vc, None, f0_shift="octave", transpose=2)
    assert conv.pitch_of() == ("octave", 2) and conv.pitch_of(None, -1) == ("octave", -1)
    assert conv.pitch_of([None, "none"], [None, 5.0], 2) == [["octave", "none"], [2, 5.0]]
    with pytest.raises(ValueError):
        conv.convert([absent, absent], transpose=[0.0])     # one value for two sources
    with pytest.raises(ValueError):
        conv.convert([absent], f0_shift="fifth")
    q = serving.RequestQueue(conv, max_wait_ms=1.0)
    try:
        with pytest.raises(ValueError):
            q.submit(absent, transpose=float("inf"))
        with pytest.raises(ValueError):
            q.submit(absent, f0_shift="fifth")
    finally:
        q.close()


def test_request_queue_hands_each_request_its_values_also_when_the_batch_is_retried_one_by_one():
    """RequestQueue._run with a stand-in converter: the batch call gets one value per request (None where the request has none),
    the retry-one-by-one path the request's own; a batch of plain requests is converted without the arguments."""
    import torch
    from concurrent.futures import Future
    from knn_svc_amd import serving

    class Conv:
        class vc:
            device = torch.device("cpu")

        def __init__(self):
            self.calls = []

        def pitch_of(self, f0_shift=None, transpose=None, n=None):
            return f0_shift, transpose

        def load_checked(self, s):
            return s, None

        def convert(self, sources, loaded=None, **kw):
            self.calls.append((list(sources), kw))
            if len(sources) > 1 and "poison" in sources:
                raise RuntimeError("the batch fails as a whole")
            return [torch.tensor([float(len(s))]) for s in sources]

    rq = serving.RequestQueue(Conv(), max_batch=3, max_wait_ms=5000.0)
    try:
        futs = [rq.submit("a", transpose=2), rq.submit("poison"), rq.submit("bcd", f0_shift="none", transpose=-1.5)]
        assert [float(f.result(timeout=30)) for f in futs] == [1.0, 6.0, 3.0]
        plain = [rq.submit("x"), rq.submit("yy"), rq.submit("zzz")]
        assert [float(f.result(timeout=30)) for f in plain] == [1.0, 2.0, 3.0]
    finally:
        rq.close()
    assert rq.batches == [3, 3] and rq.isolated == 1
    assert rq.conv.calls == [
        (["a", "poison", "bcd"], dict(f0_shift=[None, None, "none"], transpose=[2, None, -1.5])),
        (["a"], dict(f0_shift=[None], transpose=[2])),
        (["poison"], dict(f0_shift=[None], transpose=[None])),
        (["bcd"], dict(f0_shift=["none"], transpose=[-1.5])),
        (["x", "yy", "zzz"], {}),
    ]


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


def _i32(v):
    return (ctypes.c_int32 * len(v))(*v)


def _f32(v):
    return (ctypes.c_float * len(v))(*v)


def test_shift_f0_seg_mode_refuses_bad_arguments_before_launching():
    lib = _lib()
    d = 256                      # a dummy, aligned, never dereferenced: every call below fails before the launch
    tab = _table([3, 4, 5])
    ok_m, ok_t = _i32([0, 1, 3]), _f32([0.0, -12.0, 36.0])

    def refused(*args, say):
        rc = lib.knnsvc_shift_f0_seg_mode(*args)
        msg = lib.knnsvc_last_error()
        assert rc != 0 and b"shift_f0_seg_mode" in msg and say in msg, (args, rc, msg)

    refused(d, tab, 3, _i32([0, 4, 0]), ok_t, d, d, d, d, None, say=b"mode 4")
    refused(d, tab, 3, _i32([0, 0, -1]), ok_t, d, d, d, None, None, say=b"mode -1")
    refused(d, tab, 3, ok_m, _f32([0.0, float("nan"), 0.0]), d, d, d, d, None, say=b"transpose")
    refused(d, tab, 3, ok_m, _f32([0.0, 0.0, 36.5]), d, d, d, d, None, say=b"transpose 36.5")
    refused(d, tab, 3, None, _f32([float("inf"), 0.0, 0.0]), d, d, d, d, None, say=b"transpose")
    refused(d, tab, 3, ok_m, _f32([0.0, -36.25, 0.0]), d, d, d, d, None, say=b"segment 1")
    refused(None, tab, 3, ok_m, ok_t, d, d, d, d, None, say=b"null")
    refused(d, tab, 3, ok_m, ok_t, None, d, d, d, None, say=b"null")
    refused(d, tab, 3, ok_m, ok_t, d, None, d, d, None, say=b"null")
    refused(d, tab, 3, ok_m, ok_t, d, d, None, d, None, say=b"null")
    refused(d, None, 3, ok_m, ok_t, d, d, d, d, None, say=b"segment table")
    for bad, n in (((ctypes.c_int64 * 3)(0, 4, 4), 2), ((ctypes.c_int64 * 2)(1, 4), 1), ((ctypes.c_int64 * 3)(0, 9, 4), 2),
                   (_table([2] * 65), 65), (tab, 0)):
        rc = lib.knnsvc_shift_f0_seg_mode(d, bad, n, None, None, d, d, d, None, None)
        assert rc != 0 and b"shift_f0_seg_mode" in lib.knnsvc_last_error(), (n, lib.knnsvc_last_error())


def test_header_table_and_version_agree():
    """The new entry point is declared, exported and bound with ten arguments; the version number other tests pin is unchanged
    (a name was added, no existing signature moved)."""
    import os
    import re
    from knn_svc_amd import _lib as L
    lib = _lib()
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "knnsvc_hip.h")).read()
    assert re.search(r"\bint knnsvc_shift_f0_seg_mode\(", src)
    for name, val in (("MEDIAN", 0), ("OCTAVE", 1), ("SEMITONE", 2), ("NONE", 3)):
        assert re.search(rf"#define KNNSVC_F0_SHIFT_{name} {val}\b", src)
    assert "#define KNNSVC_F0_TRANSPOSE_MAX 36.0f" in src
    assert len(L.SIGNATURES["knnsvc_shift_f0_seg_mode"][1]) == 10 and hasattr(lib, "knnsvc_shift_f0_seg_mode")
    assert lib.knnsvc_abi_version() == L.ABI_VERSION


# ---------------------------------------------------------------- the oracle and the pinned inputs
def test_oracle_cases_stand_clear_of_every_rounding_tie():
    want = {"up": (1, 14), "down": (-1, -14), "near": (0, 1)}
    for name, (src, pool, _why) in O.cases().items():
        qm, pm = O.lower_median_log(src), O.lower_median_log(pool)
        far_oct, far_semi = O.tie_distance(qm, pm)
        assert far_oct >= 0.1 and far_semi >= 0.1, (name, far_oct, far_semi)
        assert len(src) % 256 != 0 and 0 < (src != 0).sum() < len(src)
        _, so = O.shift(src, qm, pm, O.OCTAVE)
        _, ss = O.shift(src, qm, pm, O.SEMITONE)
        assert (float(so) / 12, float(ss)) == want[name], (name, so, ss)
    assert max(len(s) for s, _p, _w in O.cases().values()) > 1024         # more than one block of 256 rows, several times


def test_oracle_properties():
    src, pool, _ = O.cases()["up"]
    qm, pm = O.lower_median_log(src), O.lower_median_log(pool)
    voiced = src != 0
    for mode in range(4):
        for t in (0.0, 3.0, -12.0, 0.5):
            out, semis = O.shift(src, qm, pm, mode, t)
            assert out.dtype == np.float32 and np.array_equal(out[~voiced].view(np.uint32), src[~voiced].view(np.uint32))
            ratio = 12 * np.log2(out[voiced].astype(np.float64) / src[voiced])
            assert np.abs(ratio - float(semis)).max() < 1e-4, (mode, t)        # every voiced frame moved by the reported interval
            whole = float(np.float32(semis) - np.float32(t))          # in fp32, the precision the interval is reported in
            if mode == O.OCTAVE:
                assert whole % 12 == 0 and whole == 12
            if mode == O.SEMITONE:
                assert whole == round(whole) == 14
            if mode == O.NONE:
                assert float(semis) == t
    # median, t = 0: the expression of knnsvc_shift_f0, step by step
    L = O.log_rn(src[voiced])
    assert np.array_equal(O.shift(src, qm, pm, O.MEDIAN)[0][voiced], O.exp_rn((L + pm).astype(np.float32) - qm))
    # 12 semitones without a shift: every voiced frame doubles
    dbl, _ = O.shift(src, qm, pm, O.NONE, 12.0)
    assert np.abs(dbl[voiced] / (2 * src[voiced]) - 1).max() <= 5e-7
    # a NaN median propagates where the medians are read, and only there
    nan = np.float32("nan")
    for mode in (O.MEDIAN, O.OCTAVE, O.SEMITONE):
        out, semis = O.shift(src, qm, nan, mode, 1.0)
        assert np.isnan(out[voiced]).all() and np.isnan(semis) and np.array_equal(out[~voiced], src[~voiced])
    out, semis = O.shift(src, nan, nan, O.NONE, 1.0)
    assert np.isfinite(out).all() and float(semis) == 1.0
    # rint rounds half to even
    assert O.interval(np.float32(0), np.float32(0), O.SEMITONE, 0)[1] == 0
    assert np.rint(0.5) == 0 and np.rint(1.5) == 2 and np.rint(-2.5) == -2
