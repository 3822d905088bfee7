"""CPU: what belongs to a source item (options.SourceKnobs: f0_shift / transpose, target_duration, blend weights) on its way
from ``BatchConverter.convert`` and ``RequestQueue.submit`` to the match functions — which match function a batch reaches and with
whose values, the one "a value for all items or one per item" helper, and the queue's fixed-shape entries.  The converter runs on
the duck-typed encoder / vocoder and the injected seams of tests/test_dist_bulk_cpu.py; every recording stand-in has the signature
of the function it replaces."""
import numpy as np
import pytest
import torch

from tests import test_dist_bulk_cpu as D

LENGTHS = (12345, 16000, 20000)


def _voice(seed, frames=100):
    """A serving.TargetVoice filled by hand: ``frames`` pool frames, no prepared kNN image."""
    from knn_svc_amd import serving
    g = torch.Generator().manual_seed(seed)
    tv = serving.TargetVoice.__new__(serving.TargetVoice)
    tv.ref_path = tv.ref_id = f"voice{seed}"
    tv.files = [tv.ref_id]
    tv.feats, tv.harm = torch.randn(frames, D.E, generator=g), torch.rand(frames, 49, generator=g)
    tv.f0 = 100.0 + 100.0 * torch.rand(frames, generator=g)
    tv.prep = None
    return tv


def _converter(monkeypatch, n_voices, **kw):
    """-> (BatchConverter on the CPU over ``n_voices`` voices, its sources, their frame counts).  The injected seams are put
    back when the test ends."""
    from knn_svc_amd import dist as kd, matching as M, serving
    from knn_svc_amd.matcher import KNeighborsVC
    for mod, names in ((M, ("side_features", "match_features", "prepare_pool", "batched_knn", "_POOL_CACHE")),
                       (kd, ("_hip_local_topk", "_hip_merge"))):
        for name in names:
            monkeypatch.setattr(mod, name, getattr(mod, name))
    D._inject()
    vc = KNeighborsVC(D.FakeEncoder(), D.FakeVocoder(), {"sampling_rate": 16000}, device="cpu")
    voices = [_voice(7 + v) for v in range(n_voices)]
    conv = serving.BatchConverter(vc, voices[0] if n_voices == 1 else voices, ckpt_type="mix", post_opt="no_post_opt", **kw)
    g = torch.Generator().manual_seed(3)
    Ts = [M.frames_of(n, vc.wavlm) for n in LENGTHS]
    sources = [(0.1 * torch.randn(n, generator=g), (120.0 + 60.0 * torch.rand(T, generator=g)).numpy()) for n, T in zip(LENGTHS, Ts)]
    return conv, sources, Ts


def _refuse(name):
    def fail(*a, **k):
        raise AssertionError(f"{name} must not be reached")
    return fail


def test_single_voice_batch_calls_match_features_per_source_with_its_own_values(monkeypatch):
    from knn_svc_amd import matching as M, ops
    conv, sources, Ts = _converter(monkeypatch, 1, f0_shift="semitone", transpose=-3.0)
    calls = []

    def match_features(query_seq, query_f0, matching_list, matching_f0, harmonics_list, ckpt_type, post_opt,
                       return_debug=False, nn32=None, nan_flags=None, pool_prep=None, synth_list=None, topk=None, f0_shift=None,
                       transpose=None):
        calls.append((int(query_seq.shape[0]), f0_shift, transpose, matching_list is conv.target.feats, nn32 is not None))
        return D._cpu_match_features(query_seq, query_f0, matching_list, matching_f0, harmonics_list, ckpt_type, post_opt, nn32=nn32)
    monkeypatch.setattr(M, "match_features", match_features)
    monkeypatch.setattr(M, "match_features_blend", _refuse("match_features_blend"))
    monkeypatch.setattr(ops, "blend_seg", _refuse("ops.blend_seg"))
    monkeypatch.setattr(ops, "shift_f0_seg_blend", _refuse("ops.shift_f0_seg_blend"))
    ys = conv.convert(sources, f0_shift=["median", None, "octave"], transpose=[0.0, 2.0, None])
    assert calls == [(Ts[0], "median", 0.0, True, True), (Ts[1], "semitone", 2.0, True, True), (Ts[2], "octave", -3.0, True, True)]
    assert [int(y.numel()) for y in ys] == [T * 320 for T in Ts]


def test_two_voice_batch_calls_match_features_blend_per_source_with_its_own_row(monkeypatch):
    from knn_svc_amd import matching as M
    conv, sources, Ts = _converter(monkeypatch, 2)
    calls = []

    def match_features_blend(query_seqs, query_f0s, voices, weights, ckpt_type, post_opt, nn32s=None, nan_flags=None, topk=None,
                             f0_shift=None, transpose=None):
        calls.append(([int(q.shape[0]) for q in query_seqs], list(weights), voices is conv.voices or list(voices) == conv.voices,
                      [[n is not None for n in per] for per in nn32s], f0_shift, transpose))
        return [(q.new_zeros(q.shape[0], D.E), q.new_zeros(q.shape[0], 49), f0) for q, f0 in zip(query_seqs, query_f0s)]
    monkeypatch.setattr(M, "match_features_blend", match_features_blend)
    monkeypatch.setattr(M, "match_features", _refuse("match_features"))
    ys = conv.convert(sources, blend=[None, [1, 3], (0, 2)])
    both = [[True], [True]]                       # every voice has weight in some source: both were searched for the batch
    assert calls == [([Ts[0]], [(0.5, 0.5)], True, both, [None], [None]), ([Ts[1]], [(0.25, 0.75)], True, both, [None], [None]),
                     ([Ts[2]], [(0.0, 1.0)], True, both, [None], [None])]
    assert [int(y.numel()) for y in ys] == [T * 320 for T in Ts]


def test_per_item_broadcasts_a_value_or_takes_one_per_item():
    from knn_svc_amd import matching as M
    from knn_svc_amd.options import per_item
    assert per_item(2.0, 3, "x") == [2.0] * 3 and per_item(None, 2, "x") == [None, None] and per_item("a", 0, "x") == []
    assert per_item([1, 2, 3], 3, "x") == [1, 2, 3] and per_item((1, None), 2, "x") == [1, None] and per_item([], 0, "x") == []
    for v, n in (([1, 2], 3), ([], 1), ((1,), 0)):
        with pytest.raises(ValueError) as e:
            per_item(v, n, "x")
        assert str(e.value) == f"x: {len(v)} values for {n} items"
    assert per_item([None, "none"], 2, "x", default="octave") == ["octave", "none"] and per_item(None, 2, "x", default=7) == [7, 7]
    assert per_item([None, 3], 2, "x", float) == [None, 3.0] and per_item([None, 3], 2, "x", float, default=-1) == [-1, 3.0]
    # weights: a flat vector is ONE value, a list of vectors and Nones (the empty list too) is one entry per item
    vec = dict(one=tuple, is_list=M.blend_per_item, unit="weight vectors")
    assert per_item([1, 3], 3, "blend", **vec) == [(1, 3)] * 3 and per_item(np.array([1, 3]), 2, "blend", **vec) == [(1, 3)] * 2
    assert per_item([[1, 3], None, (0, 2)], 3, "blend", default=(5, 5), **vec) == [(1, 3), (5, 5), (0, 2)]
    assert per_item([None, None], 2, "blend", **vec) == [None, None] and per_item([], 0, "blend", **vec) == []
    for v, n in (([[1, 3]], 2), ([None, [1, 3]], 1), ([], 2)):
        with pytest.raises(ValueError) as e:
            per_item(v, n, "blend", **vec)
        assert str(e.value) == f"blend: {len(v)} weight vectors for {n} items"


def test_request_queue_round_trip_hands_on_only_the_knobs_a_batch_carries():
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
            return tuple(b)

        def plan_duration(self, w, d, item=None):
            pass

        def load_checked(self, s):
            return s, None

        def convert(self, sources, loaded=None, **kw):
            self.calls.append((list(sources), kw))
            return [torch.tensor([float(len(s))]) for s in sources]

    conv = Conv()
    for max_batch, submits in ((4, (("a", {}), ("bb", dict(transpose=2.0)), ("ccc", dict(target_duration=1.5)), ("dddd", dict(blend=[1, 3])))),
                               (2, (("x", {}), ("yy", {})))):
        rq = serving.RequestQueue(conv, max_batch=max_batch, max_wait_ms=5000.0)
        try:
            futs = [rq.submit(s, **kw) for s, kw in submits]
            assert [float(f.result(timeout=30)) for f in futs] == [float(len(s)) for s, _ in submits]
        finally:
            rq.close()
        assert rq.batches == [max_batch] and rq.isolated == 0
    assert conv.calls == [
        (["a", "bb", "ccc", "dddd"], dict(f0_shift=[None] * 4, transpose=[None, 2.0, None, None],
                                          target_duration=[None, None, 1.5, None], blend=[None, None, None, (1, 3)])),
        (["x", "yy"], {}),
    ]
