"""CPU: voice blending without a GPU — matching.resolve_blend, the oracle's own properties (tests/blend_oracle.py), the C ABI of
knnsvc_blend_seg and knnsvc_shift_f0_seg_blend (every argument is checked before the launch, so dummy pointers are never
dereferenced), the command line and the entry points' refusals before a file is read."""
import ctypes
import dataclasses
import math

import numpy as np
import pytest
import torch

import blend_oracle as O


# ---------------------------------------------------------------- resolve_blend
def test_resolve_blend_normalises_in_fp64():
    from knn_svc_amd import matching as M
    assert M.resolve_blend([7, 3], 2) == (0.7, 0.3) == O.normalise([7, 3])
    assert M.resolve_blend((0.5, 0.25, 0.25), 3) == (0.5, 0.25, 0.25)
    a = M.resolve_blend([0.3, 0.7], 2)
    assert a == O.normalise([0.3, 0.7]) and a[::-1] == M.resolve_blend([0.7, 0.3], 2)      # fsum: the order does not matter
    a = M.resolve_blend(np.array([1, 2, 3, 4], np.float32), 4)
    assert a == tuple(w / 10.0 for w in (1.0, 2.0, 3.0, 4.0)) and abs(math.fsum(a) - 1.0) < 1e-15
    assert M.resolve_blend([np.float32(2), np.int64(2)], 2) == (0.5, 0.5)
    assert all(O.check_row(M.resolve_blend(v, len(v))) is None for v in ([1e-300, 1e300], [3, 3, 3], [1e-3, 5, 7, 11]))


def test_resolve_blend_keeps_a_one_hot_vector_exactly_one_hot():
    from knn_svc_amd import matching as M
    for V in (2, 3, 4):
        for hot in range(V):
            for scale in (1, 0.3, 7.5, 1e-30):
                v = [0.0] * V
                v[hot] = scale
                got = M.resolve_blend(v, V)
                assert got == tuple(1.0 if i == hot else 0.0 for i in range(V)), (v, got)
    assert str(M.resolve_blend([-0.0, 2], 2)[0]) == "0.0"


def test_resolve_blend_none_means_equal_weights():
    from knn_svc_amd import matching as M
    assert M.resolve_blend(None, 2) == (0.5, 0.5) and M.resolve_blend(None, 4) == (0.25,) * 4
    assert M.resolve_blend(None, 3) == (1.0 / 3,) * 3 and O.check_row(M.resolve_blend(None, 3)) is None
    assert M.resolve_blend(None, 2, 3) == [(0.5, 0.5)] * 3


def test_resolve_blend_per_item():
    from knn_svc_amd import matching as M
    assert M.resolve_blend([1, 3], 2, 3) == [(0.25, 0.75)] * 3                    # one vector for all items
    assert M.resolve_blend([[1, 3], None, (1, 0)], 2, 3) == [(0.25, 0.75), (0.5, 0.5), (1.0, 0.0)]
    assert M.resolve_blend([[1, 1]], 2, 1) == [(0.5, 0.5)] and M.resolve_blend([], 2, 0) == []
    assert M.resolve_blend([1, 1], 2, 2) == [(0.5, 0.5)] * 2                       # numbers: a vector, not two items


@pytest.mark.parametrize("v", [[1.0], [1, 2, 3], [-1, 2], [float("nan"), 1], [float("inf"), 1], [0, 0], [0.0, -0.0], [True, 1],
                               ["1", 1], "1,1", 0.5, {0: 1, 1: 1}, [[1, 1]], [None, 1], [1e308, 1e308]])
def test_resolve_blend_refuses(v):
    from knn_svc_amd import matching as M
    with pytest.raises(ValueError):
        M.resolve_blend(v, 2)


def test_resolve_blend_refuses_voice_counts_and_item_counts():
    from knn_svc_amd import matching as M
    for n in (0, 1, 5, True, 2.5):
        with pytest.raises(ValueError):
            M.resolve_blend(None, n)
    for v in ([[1, 1], [1, 1]], [[1, 1], None, None, None], [[1, 1], [1, 2, 3], None], [[1, 1], [-1, 2], None], [None, None, "x"]):
        with pytest.raises(ValueError):
            M.resolve_blend(v, 2, 3)
    assert (M.BLEND_MAX_VOICES, O.MAX_VOICES) == (4, 4)


# ---------------------------------------------------------------- the oracle's own properties
def test_oracle_swapping_two_voices_and_their_weights_gives_the_same_bits():
    a, b = O.feats(40, 33, 1), O.feats(40, 33, 2)
    for w in ((0.3, 0.7), (0.5, 0.5), O.normalise([1, 1e-3]), (1.0, 0.0)):
        x, y = O.blend([a, b], w), O.blend([b, a], w[::-1])
        assert x.dtype == np.float32 and np.array_equal(x.view(np.uint32), y.view(np.uint32))
    assert not np.array_equal(O.blend([a, b], (0.3, 0.7)), O.blend([a, b], (0.7, 0.3)))


def test_oracle_a_zero_weight_voice_full_of_nan_changes_nothing():
    a, b, c = O.feats(20, 7, 3), O.feats(20, 7, 4), np.full((20, 7), np.nan, np.float32)
    want = O.blend([a, b], (0.25, 0.75))
    assert np.array_equal(O.blend([a, c, b], (0.25, 0.0, 0.75)).view(np.uint32), want.view(np.uint32))
    assert np.array_equal(O.blend([c, a, b, c], (0.0, 0.25, 0.75, 0.0)).view(np.uint32), want.view(np.uint32))
    assert np.isnan(O.blend([a, c, b], (0.25, 1e-9, 0.75 - 1e-9))).all()              # any weight above 0 lets it through
    one = O.blend([c, a], (0.0, 1.0))
    assert np.array_equal(one.view(np.uint32), a.view(np.uint32)) and one is not a      # a single term: a copy, bit for bit
    odd = np.array([[-0.0, np.float32("nan"), 1e-45]], np.float32)
    assert np.array_equal(O.blend([odd, odd], (1.0, 0.0)).view(np.uint32), odd.view(np.uint32))


def test_oracle_is_the_fp64_sum_rounded_once_and_the_median_follows_the_same_rule():
    a, b, c = (O.feats(9, 5, s) for s in (5, 6, 7))
    w = O.normalise([2, 3, 5])
    want = ((np.float64(w[0]) * a.astype(np.float64) + np.float64(w[1]) * b.astype(np.float64)) + np.float64(w[2]) * c.astype(np.float64))
    assert np.array_equal(O.blend([a, b, c], w), want.astype(np.float32))
    seg = O.table([2, 3, 4])
    rows = [w, (0.0, 1.0, 0.0), (0.5, 0.0, 0.5)]
    out = O.blend_seg([a, b, c], seg, rows)
    assert np.array_equal(out[2:5], b[2:5]) and np.array_equal(out[:2], O.blend([a[:2], b[:2], c[:2]], w))
    pms = [np.float32(4.7), np.float32(5.4), np.float32("nan")]
    assert O.median(pms, (0.5, 0.5, 0.0)) == np.float32(0.5 * np.float64(pms[0]) + 0.5 * np.float64(pms[1]))
    assert O.median(pms, (0.0, 1.0, 0.0)) == pms[1] and np.isnan(O.median(pms, (0.5, 0.25, 0.25)))
    assert [O.check_row(r) for r in ((0.5, 0.5), (1.0,), (0.5, -0.5, 1.0), (0.0, 0.0), (0.6, 0.6), (float("nan"), 1.0), (float("inf"), 0.0))] == \
        [None, "voices", "entry", "no positive", "sum", "entry", "entry"]


# ---------------------------------------------------------------- the C ABI
def _lib():
    import __graft_entry__ as g
    g.build()
    from knn_svc_amd import _lib
    return _lib.load()


def _table(lens):
    return (ctypes.c_int64 * (len(lens) + 1))(*O.table(lens))


def _f64(v):
    return (ctypes.c_double * len(v))(*v)


BAD_ROWS = [([0.5, 0.5, 1.5, -0.5], b"segment 1"), ([0.5, 0.5, float("nan"), 1.0], b"segment 1"), ([0.0, 0.0, 0.5, 0.5], b"segment 0"),
            ([0.5, 0.5, 0.6, 0.6], b"segment 1"), ([0.5, 0.5, 2.0, 3.0], b"sum"), ([float("inf"), 0.0, 0.5, 0.5], b"segment 0"),
            ([0.5, 0.5 + 3e-6, 0.5, 0.5], b"segment 0")]


def test_blend_seg_refuses_bad_arguments_before_launching():
    lib = _lib()
    d = 256                      # a dummy, aligned, never dereferenced: every call below fails before the launch
    ptrs = lambda n, v=d: (ctypes.c_void_p * n)(*([v] * n))
    seg, ok = _table([3, 4]), _f64([0.5, 0.5, 0.25, 0.75])

    def refused(*args, say):
        rc = lib.knnsvc_blend_seg(*args)
        msg = lib.knnsvc_last_error()
        assert rc != 0 and b"blend_seg" in msg and say in msg, (args, rc, msg)

    refused(None, 2, 8, seg, 2, ok, d, None, say=b"null")
    refused(ptrs(2), 2, 8, seg, 2, ok, None, None, say=b"null")
    refused(ptrs(2), 2, 8, seg, 2, None, d, None, say=b"weight")
    refused((ctypes.c_void_p * 2)(d, None), 2, 8, seg, 2, ok, d, None, say=b"voice 1")
    refused(ptrs(2), 2, 8, None, 2, ok, d, None, say=b"segment table")
    refused(ptrs(1), 1, 8, seg, 2, ok, d, None, say=b"n_voices")
    refused(ptrs(5), 5, 8, seg, 2, _f64([0.2] * 10), d, None, say=b"n_voices")
    refused(ptrs(2), 2, 0, seg, 2, ok, d, None, say=b"dim")
    for row, say in BAD_ROWS:
        refused(ptrs(2), 2, 8, seg, 2, _f64(row), d, None, say=say)
    for bad, n in (((ctypes.c_int64 * 3)(0, 4, 4), 2), ((ctypes.c_int64 * 2)(1, 4), 1), (_table([2] * 65), 65), (seg, 0)):
        rc = lib.knnsvc_blend_seg(ptrs(2), 2, 8, bad, n, _f64([0.5, 0.5] * max(n, 1)), d, None)
        assert rc != 0 and b"blend_seg" in lib.knnsvc_last_error(), (n, lib.knnsvc_last_error())


def test_shift_f0_seg_blend_refuses_bad_arguments_before_launching():
    lib = _lib()
    d = 256
    seg, ok = _table([3, 4]), _f64([0.5, 0.5, 0.25, 0.75])

    def refused(*args, say):
        rc = lib.knnsvc_shift_f0_seg_blend(*args)
        msg = lib.knnsvc_last_error()
        assert rc != 0 and b"shift_f0_seg_blend" in msg and say in msg, (args, rc, msg)

    for hole in (0, 5, 6, 9):                          # f0, query_median, pool_medians, shifted
        args = [d, seg, 2, None, None, d, d, 2, ok, d, None, None]
        args[hole] = None
        refused(*args, say=b"null")
    refused(d, seg, 2, None, None, d, d, 2, None, d, None, None, say=b"weight")
    refused(d, None, 2, None, None, d, d, 2, ok, d, None, None, say=b"segment table")
    refused(d, seg, 2, None, None, d, d, 1, ok, d, None, None, say=b"n_voices")
    refused(d, seg, 2, None, None, d, d, 5, _f64([0.2] * 10), d, None, None, say=b"n_voices")
    for row, say in BAD_ROWS:
        refused(d, seg, 2, None, None, d, d, 2, _f64(row), d, None, None, say=say)
    refused(d, seg, 2, (ctypes.c_int32 * 2)(0, 4), None, d, d, 2, ok, d, None, None, say=b"mode")
    refused(d, seg, 2, None, (ctypes.c_float * 2)(0.0, 40.0), d, d, 2, ok, d, None, None, say=b"transpose")
    for bad, n in (((ctypes.c_int64 * 3)(0, 4, 4), 2), ((ctypes.c_int64 * 2)(1, 4), 1), (_table([2] * 65), 65), (seg, 0)):
        rc = lib.knnsvc_shift_f0_seg_blend(d, bad, n, None, None, d, d, 2, _f64([0.5, 0.5] * max(n, 1)), d, None, None)
        assert rc != 0 and b"shift_f0_seg_blend" in lib.knnsvc_last_error(), (n, lib.knnsvc_last_error())


def test_header_table_and_library_agree_on_both_entries():
    import os
    import re
    from knn_svc_amd import _lib as L, ops
    lib = _lib()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = open(os.path.join(root, "include", "knnsvc_hip.h")).read()
    assert re.search(r"\bint knnsvc_blend_seg\(", src) and re.search(r"\bint knnsvc_shift_f0_seg_blend\(", src) and "Voice blend" in src
    assert re.search(r"#define KNNSVC_BLEND_MAX_VOICES 4\b", src) and ops.BLEND_MAX_VOICES == 4
    res, args = L.SIGNATURES["knnsvc_blend_seg"]
    assert res is ctypes.c_int32 and len(args) == 8 and args[1] is args[2] is args[4] is ctypes.c_int32
    res, args = L.SIGNATURES["knnsvc_shift_f0_seg_blend"]
    assert res is ctypes.c_int32 and len(args) == 12 and args[2] is args[7] is ctypes.c_int32
    assert hasattr(lib, "knnsvc_blend_seg") and hasattr(lib, "knnsvc_shift_f0_seg_blend")
    assert "blend.hip" in open(os.path.join(root, "knn_svc_amd", "csrc", "Makefile")).read()
    assert lib.knnsvc_abi_version() == L.ABI_VERSION


def test_ops_refuse_cpu_tensors_and_bad_shapes():
    from knn_svc_amd import ops
    x = torch.zeros(4, 8)
    with pytest.raises(ops.KnnSvcError):
        ops.blend_seg([x, x], [0, 4], [(0.5, 0.5)])
    with pytest.raises(ops.KnnSvcError):
        ops.blend_seg([], [0, 4], [()])
    with pytest.raises(ops.KnnSvcError):
        ops.shift_f0_seg_blend(torch.zeros(4), [0, 4], torch.zeros(1, 2), torch.zeros(2, 2), [(0.5, 0.5)])
    for rows, nv in (([(0.5, 0.5)], 2), ([(1.0,), (1.0,)], 1), ([(0.2,) * 5] * 2, 5), ([(0.5, 0.5), (1.0, 0.0, 0.0)], 2)):
        with pytest.raises(ops.KnnSvcError):
            ops._blend_rows("blend_seg", rows, 2, nv)
    assert ops._blend_rows("blend_seg", [[0.5, 0.5], (1, 0)], 2, 2) == [(0.5, 0.5), (1.0, 0.0)]


# ---------------------------------------------------------------- the record, the command line, the entry points
def test_extensions_record_is_unchanged_and_the_cli_defaults_are_none():
    from knn_svc_amd.inference import build_parser
    from knn_svc_amd.options import Extensions
    assert [f.name for f in dataclasses.fields(Extensions)] == ["topk", "vad_level", "f0_shift", "transpose", "loudness_db",
                                                                "envelope_mix", "peak_db"]
    ap = build_parser()
    a = ap.parse_args(["s", "t"])
    assert a.blend_tgt is None and a.blend is None
    a = ap.parse_args(["s", "t", "--blend_tgt", "u", "--blend_tgt", "v", "--blend", "0.5,0.25,0.25"])
    assert a.blend_tgt == ["u", "v"] and a.blend == [0.5, 0.25, 0.25]


def test_main_refuses_before_loading_anything(tmp_path):
    from knn_svc_amd import inference
    absent = [str(tmp_path / "absent.wav"), str(tmp_path / "absent2.wav")]
    other = str(tmp_path / "absent3.wav")
    for extra in (["--blend", "0.5,0.5"],                                                   # weights without voices
                  ["--blend_tgt", other, "--blend", "1"], ["--blend_tgt", other, "--blend", "1,1,1"],      # a count that does not match
                  ["--blend_tgt", other, "--blend", "1,-1"], ["--blend_tgt", other, "--blend", "0,0"],
                  ["--blend_tgt", other, "--blend", "nan,1"], ["--blend_tgt", other, "--blend", "a,b"],
                  ["--blend_tgt", other] * 4):                                             # five voices
        with pytest.raises(SystemExit) as e:
            inference.main(absent + extra)
        assert e.value.code == 2, extra
    (tmp_path / "A").mkdir(); (tmp_path / "B").mkdir()
    for extra in (["--blend", "0.5,0.5"], ["--blend_tgt", other], ["--blend_tgt", other, "--blend", "0.5,0.5"]):      # folder mode
        with pytest.raises(SystemExit) as e:
            inference.main([str(tmp_path / "A"), str(tmp_path / "B")] + extra)
        assert e.value.code == 2, extra


def test_entry_points_refuse_before_a_file_is_read(tmp_path, monkeypatch):
    from knn_svc_amd import serving
    from knn_svc_amd.matcher import KNeighborsVC
    vc = KNeighborsVC.__new__(KNeighborsVC)                 # no models: nothing below may get as far as using one
    vc.device = torch.device("cpu")
    absent = str(tmp_path / "absent.wav")
    bad = (dict(blend=[0.5, 0.5]),                                           # blend without several voices
           dict(blend_with=absent, blend=[1.0]), dict(blend_with=[absent], blend=[1, 1, 1]),      # a wrong count of weights
           dict(blend_with=[absent] * 4), dict(blend_with=[]),               # more than four voices, none
           dict(blend_with=absent, blend=[1, -1]), dict(blend_with=absent, blend=[0, 0]), dict(blend_with=absent, blend="1,1"))
    for kw in bad:
        with pytest.raises(ValueError):
            vc.special_match(absent, absent, **kw)
        with pytest.raises(ValueError):
            vc.many_to_one([absent], absent, **kw)
    monkeypatch.setenv("KNNSVC_POOL_SHARD", "1")            # a blend under a sharded pool
    for fn in (lambda: vc.special_match(absent, absent, blend_with=absent), lambda: vc.many_to_one([absent], absent, blend_with=[absent]),
               lambda: serving.BatchConverter(vc, [None, None])):
        with pytest.raises(ValueError) as e:
            fn()
        assert "KNNSVC_POOL_SHARD" in str(e.value)
    monkeypatch.delenv("KNNSVC_POOL_SHARD")
    for target, kw in ((None, dict(blend=[0.5, 0.5])), ([None], {}), ([None] * 5, {}), ([None, None], dict(blend=[1, 1, 1])),
                       ([None, None], dict(blend=[1, float("nan")]))):
        with pytest.raises(ValueError):
            serving.BatchConverter(vc, target, **kw)
    one = serving.BatchConverter(vc, None)
    assert one.voices is None and one.blend_of() is None and one.blend_of(None, 3) is None and one.blend_of([None, None], 2) is None
    with pytest.raises(ValueError):
        one.convert([absent], blend=[0.5, 0.5])
    two = serving.BatchConverter(vc, [None, None], blend=[3, 1])
    assert two.blend == (0.75, 0.25) and two.blend_of() == (0.75, 0.25) and two.blend_of([1, 1]) == (0.5, 0.5)
    assert two.blend_of(None, 2) == [(0.75, 0.25)] * 2 and two.blend_of([1, 0], 2) == [(1.0, 0.0)] * 2
    assert two.blend_of([None, [1, 3], (0, 2)], 3) == [(0.75, 0.25), (0.25, 0.75), (0.0, 1.0)]
    assert serving.BatchConverter(vc, (None, None, None)).blend == (1.0 / 3,) * 3
    for v in ([1.0], [1, 1, 1], [[1, 1]], [1, -1], "x"):
        with pytest.raises(ValueError):
            two.convert([absent], blend=v if v != [[1, 1]] else [[1, 1], [1, 1]])
    q = serving.RequestQueue(two, max_wait_ms=1.0)
    try:
        for v in ([1.0], [1, 1, 1], [0, 0], [1, float("inf")], "x"):
            with pytest.raises(ValueError):
                q.submit(absent, blend=v)
    finally:
        q.close()


def test_request_queue_hands_each_request_its_weights():
    """RequestQueue._run with a stand-in converter: requests with and without weights of their own share a batch, and the batch
    call gets one entry per request (None: the converter's default)."""
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

        def blend_of(self, b=None, n=None):
            if len(b) != 2:
                raise ValueError("count")
            return tuple(b)

        def plan_duration(self, w, d, item=None):
            pass

        def load_checked(self, s):
            return s, None

        def convert(self, sources, loaded=None, **kw):
            self.calls.append((list(sources), kw))
            return [torch.tensor([float(len(s))]) for s in sources]

    rq = serving.RequestQueue(Conv(), max_batch=3, max_wait_ms=5000.0)
    try:
        with pytest.raises(ValueError):
            rq.submit("zz", blend=[1.0])                   # fails alone, at the door
        futs = [rq.submit("a", blend=[0.7, 0.3]), rq.submit("bb"), rq.submit("ccc", blend=[0.0, 1.0], target_duration=2.0)]
        assert [float(f.result(timeout=30)) for f in futs] == [1.0, 2.0, 3.0]
    finally:
        rq.close()
    assert rq.batches == [3] and rq.isolated == 0
    assert rq.conv.calls == [(["a", "bb", "ccc"], dict(target_duration=[None, None, 2.0], blend=[(0.7, 0.3), None, (0.0, 1.0)]))]
