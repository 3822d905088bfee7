"""CPU: the pool-silence trimmer without a GPU — the fp64 oracle (tests/vad_oracle.py) in its two formulations, the constants at
16 kHz, the margin that makes the GPU comparison in tests/test_gpu_vad.py an exact one, the host side of the C ABI (workspace
size, refusals before any launch), the bookkeeping of matching.get_complete_spk_pool (f0 slicing, cache keys) and the switches of
the command line and the Python entry points.  The oracle restates the sox `vad` effect with torchaudio's defaults
(include/knnsvc_hip.h); neither is available here, parity with torchaudio's own code is not pinned."""
import ctypes
import inspect
import math

import numpy as np
import pytest

import vad_cases as VC
import vad_oracle as O


@pytest.fixture(scope="module")
def cases():
    return VC.cases()


@pytest.fixture(scope="module")
def trims(cases):
    """name -> ((lstrip, rstrip), details) by the vectorised formulation, computed once."""
    return {name: O.trim(x, level, details=True) for name, (x, level) in cases.items()}


def test_constants_at_16_khz():
    k = O.constants(16000)
    got = tuple(k[n] for n in ("measure_len", "dft_len", "period", "s0", "s1", "c0", "c1"))
    assert got == (1600, 2048, 800, 6, 768, 4, 53)
    assert (k["smooth"], k["up"], k["down"], k["trig"]) == (math.exp(-1 / 8), math.exp(-1 / 2), math.exp(-5), math.exp(-1 / 5))
    # periodic Hann: zero at 0, the peak 2 / sqrt(n) in the middle, win[1] == win[n - 1] (denominator n, not n - 1)
    assert k["win"][0] == 0 and abs(k["win"][800] - 2 / 40) < 1e-15 and abs(k["win"][1] - k["win"][1599]) < 1e-15
    assert k["cwin"].size == 762 and abs(k["cwin"][381] - 2 / math.sqrt(762)) < 1e-15
    assert [O.n_measurements(n, k) for n in (1599, 1600, 2399, 2400, 32000)] == [0, 1, 1, 2, 39]


def test_constants_follow_the_rate():
    k = O.constants(8000)
    assert tuple(k[n] for n in ("measure_len", "dft_len", "period", "s0", "s1", "c0", "c1")) == (800, 1024, 400, 6, 512, 2, 26)


def test_both_formulations_agree_on_every_case(cases, trims):
    for name, (x, level) in cases.items():
        assert O.streaming_trim(x, level) == trims[name][0], name


def test_expected_cuts(trims):
    """What the cases were built to reach (measurement period 800, hop 320)."""
    for n in (1599, 1600, 2399, 2400):
        assert trims[f"n{n}"][0] == (-1, -1)                       # never past the boot phase
    assert trims["tone2s/3"][0] == trims["tone2s/7"][0] == (8000, 6400)
    assert trims["tone2s/12"][0] == (-1, -1)                       # the running mean never gets there
    assert trims["tone2s/7"][1]["fwd"].size == 39
    assert trims["early-burst"][0][0] == 4160                      # 5 x 800 (the last boot measurement) rounded up to a hop
    assert trims["two-bursts/gap3"][0][0] == 8000                  # in front of the FIRST burst (at 9600)
    assert trims["two-bursts/gap8"][0][0] == 16960                 # in front of the second: 21 x 800 rounded up
    (l, r), d = trims["short-voiced"]
    assert l > 0 and r > 0 and 0 < d["m_rev"] < d["rev"].size      # the reversed scan sees fewer measurements than exist
    (l, r), d = trims["golden-tgt"]
    assert l >= 0 and l % 320 == 0 and r % 320 == 0


def test_every_measure_of_the_boot_phase_is_zero(trims):
    for name, (_res, d) in trims.items():
        for v in (d["fwd"], d["rev"]):
            assert np.all(v[:O.BOOT_COUNT_MAX] == 0.0), name
            assert np.all(v >= 0.0), name
    assert any(np.any(d["fwd"][O.BOOT_COUNT_MAX:] > 0) for _r, d in trims.values())


@pytest.mark.parametrize("make", [lambda: np.zeros(32000, np.float32), lambda: np.full(32000, 0.5, np.float32)])
def test_silence_and_dc_never_trigger(make):
    x = make()
    assert np.all(O.measures(x) == 0.0) and np.all(O.measures(x, reverse=True) == 0.0)
    assert O.trim(x, 1e-2) == (-1, -1) and O.streaming_trim(x, 1e-2) == (-1, -1)


def test_margin_condition(trims):
    """No decision of any case the GPU test runs stands closer than 1e-6 to flipping: the running mean against the level at every
    step up to the trigger, every walked-back measure against the level, every walked-back measure against 0.  Measures that
    agree with the oracle's within 1e-6 therefore give exactly its cut points."""
    for name, (_res, d) in trims.items():
        assert d["margin"] >= VC.MARGIN, (name, d["margin"])


def test_the_8_khz_case_keeps_the_margin_too():
    x, level, sr = VC.tone_8k()
    res, d = O.trim(x, level, sr, details=True)
    assert d["margin"] >= VC.MARGIN and res != (-1, -1) and d["fwd"].size == 39, (res, d["margin"])
    assert O.streaming_trim(x, level, sr) == res


class _Enc:
    """The frame law of the encoder without its weights."""
    def __init__(self):
        from knn_svc_amd import config as C
        self.conv = [dict(k=k, s=s) for _dim, k, s in C.conv_layers(C.WAVLM_LARGE)]
        self.n_layers, self.uid, self.layer_mix = 6, 1, None

    def n_frames(self, n):
        from knn_svc_amd.wavlm import WavLMEncoder
        return WavLMEncoder.n_frames(self, n)

    def weights_fingerprint(self):
        return "abc"


def test_cuts_are_whole_hops_and_the_sliced_f0_covers_the_frames():
    from knn_svc_amd import matching
    enc = _Enc()
    for L in (6400, 6401, 20800, 33333, 480000, 480321, 481000):
        f0 = np.arange(L // 320 + 1, dtype=np.float32)               # one value per hop of the UNTRIMMED file
        assert len(f0) >= matching.frames_of(L, enc)
        for start, rstart in ((0, 0), (1, 1), (319, 321), (4000, 800), (4160, 4160)):
            l, r = O._round_up(start), O._round_up(rstart)
            assert l % 320 == 0 and r % 320 == 0 and 0 <= l - start < 320
            if L - l - r < 1600:
                continue
            T = matching.frames_of(L - l - r, enc)
            cut = matching.slice_f0(f0, l, T)
            assert T <= len(cut) <= T + 1 and cut[0] == l // 320, (L, l, r, T, len(cut))
    with pytest.raises(AssertionError):
        matching.slice_f0(np.zeros(10), 100, 3)


def test_cache_keys_move_only_when_trimming_is_on():
    from knn_svc_amd import matching
    enc = _Enc()
    assert matching.vad_tag(0) == () and matching.vad_tag(None) == () and matching.vad_tag(1e-3) == ()
    assert not matching.vad_active(0) and not matching.vad_active(1e-3) and matching.vad_active(7)
    base = (enc.weights_fingerprint(), enc.n_layers, None)
    assert matching.disk_identity(enc) == base == matching.disk_identity(enc, 0)
    assert matching.disk_identity(enc, 7) == base + (("vad", 7.0),)
    assert matching.disk_identity(enc, 7) != matching.disk_identity(enc, 3)


def _lib():
    import __graft_entry__ as g
    g.build()
    from knn_svc_amd import _lib
    return _lib.load()


def test_workspace_size_is_host_side():
    lib = _lib()
    sizes = [lib.knnsvc_vad_workspace_bytes(n, 1, 16000) for n in (1, 1600, 32000, 480000, 9600000)]
    assert all(s > 0 for s in sizes) and sizes == sorted(sizes), sizes
    k = O.constants(16000)
    rows = 32000 // 800 + 1
    assert sizes[2] == 8 * (4 * 1024 + 1600 + 762 + 2 * rows * 762 + 2 * rows)
    assert lib.knnsvc_vad_workspace_bytes(32000, 1, 8000) > 0
    assert lib.knnsvc_vad_workspace_bytes(32000, 1, 48000) == 0 and b"sample rate" in lib.knnsvc_last_error()
    assert lib.knnsvc_vad_workspace_bytes(0, 1, 16000) == 0 and b"length" in lib.knnsvc_last_error()
    assert lib.knnsvc_vad_workspace_bytes(32000, 65, 16000) == 0 and b"n_seg" in lib.knnsvc_last_error()
    assert k["s1"] - k["s0"] == 762


def test_trim_refuses_before_it_launches():
    """Dummy pointers, never dereferenced: every refusal below happens on the host, before the first launch."""
    lib = _lib()
    p = ctypes.c_void_p(256)
    tab = (ctypes.c_int64 * 2)(0, 32000)
    big = lib.knnsvc_vad_workspace_bytes(32000, 1, 16000)
    call = lambda wav=p, seg=tab, n=1, sr=16000, level=7.0, out=p, ws=p, nbytes=big: \
        lib.knnsvc_vad_trim_seg(wav, seg, n, sr, level, out, None, ws, nbytes, None)
    assert call(nbytes=big - 1) != 0 and b"workspace" in lib.knnsvc_last_error()
    assert call(sr=48000) != 0 and b"sample rate" in lib.knnsvc_last_error()
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        assert call(level=bad) != 0 and b"level" in lib.knnsvc_last_error()
    assert call(out=None) != 0 and b"null" in lib.knnsvc_last_error()
    assert call(seg=(ctypes.c_int64 * 2)(0, 0)) != 0 and b"ascending" in lib.knnsvc_last_error()
    assert call(seg=None) != 0 and b"segment table" in lib.knnsvc_last_error()


def test_ops_refuse_cpu_tensors_and_bad_levels():
    import torch
    from knn_svc_amd import ops
    from knn_svc_amd._lib import KnnSvcError
    with pytest.raises(KnnSvcError):
        ops.vad_trim(torch.zeros(8000), 7)
    with pytest.raises(KnnSvcError):
        ops.vad_trim([torch.zeros(8000)], 7)
    with pytest.raises(KnnSvcError):
        ops.vad_trim([], 7)


def test_cli_switch():
    from knn_svc_amd.inference import build_parser
    a = build_parser().parse_args(["s", "t"])
    assert a.use_vad is False and a.vad_trigger_level == 7
    a = build_parser().parse_args(["s", "t", "--use_vad", "true"])
    assert a.use_vad is True and a.vad_trigger_level == 7
    a = build_parser().parse_args(["s", "t", "--use_vad", "true", "--vad_trigger_level", "4.5"])
    assert a.use_vad is True and a.vad_trigger_level == 4.5


def test_entry_points_carry_the_switch_off_by_default():
    from knn_svc_amd import matching, ops, serving
    from knn_svc_amd.matcher import KNeighborsVC
    par = lambda fn: inspect.signature(fn).parameters
    for fn in (KNeighborsVC.special_match, KNeighborsVC.bulk_match, matching.match_at_inference_time):
        assert par(fn)["use_vad"].default is False and par(fn)["vad_trigger_level"].default == 7
    assert par(KNeighborsVC.many_to_one)["vad_trigger_level"].default is None
    assert par(serving.TargetVoice.__init__)["vad_trigger_level"].default is None
    assert par(matching.get_complete_spk_pool)["vad_trigger_level"].default == 0
    assert list(par(ops.vad_trim))[:2] == ["wavs", "trigger_level"]
    assert par(ops.vad_trim)["sample_rate"].default == 16000 and par(ops.vad_trim)["return_measures"].default is False
