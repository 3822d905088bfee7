"""CPU: the loudness feature without a GPU — the fp64 oracle (tests/loudness_oracle.py) on anchors worked out once, the host side
of the C ABI (workspace size, refusals before any launch), and the switches of the command line and the Python entry points."""
import ctypes
import inspect
import math

import numpy as np
import pytest

import loudness_oracle as O


def _sine(sr):
    return np.sin(2 * np.pi * 997 * np.arange(3 * sr) / sr).astype(np.float32)


def _impulse():
    x = np.zeros(8000, np.float32)
    x[0] = 1.0
    return x


def test_oracle_coefficients_at_16_khz():
    (sb, sa), (hb, ha) = O.coefficients(16000)
    assert np.allclose(sb, [1.444233908713844, -1.839542987741787, 0.685432300820589], rtol=0, atol=1e-14)
    assert np.allclose(sa, [1, -1.1071392365035588, 0.3972624582962044], rtol=0, atol=1e-14)
    assert np.allclose(hb, [0.9852425301500196, -1.9704850603000392, 0.9852425301500196], rtol=0, atol=1e-14)
    assert np.allclose(ha, [1, -1.9703753578723906, 0.9705947627276879], rtol=0, atol=1e-14)


@pytest.mark.parametrize("sr,expected", [(16000, -3.0832157), (48000, -3.0516807)])
def test_oracle_full_scale_997_hz_sine(sr, expected):
    lk = O.loudness(_sine(sr), sr)
    assert abs(lk - expected) < 1e-6 and abs(lk - (-3.01)) < 0.1            # BS.1770: a full-scale 997 Hz sine reads -3.01


@pytest.mark.parametrize("name,make,expected,counts", [
    ("impulse", _impulse, -35.4020140, (2, 1, 1)),
    ("constant", lambda: np.full(16000, 0.5, np.float32), -32.3337576, (7, 1, 1)),
    ("gated", O.gated_signal, -14.9031061, (27, 24, 20)),
])
def test_oracle_anchors(name, make, expected, counts):
    lk, got, margin = O.loudness(make(), 16000, details=True)
    assert abs(lk - expected) < 1e-6 and got == counts, (name, lk, got)
    assert margin > 1.0, margin                                              # no gate decision of an anchor is a close call


def test_oracle_without_blocks_or_energy():
    short = (0.2 * np.random.default_rng(1).standard_normal(6399)).astype(np.float32)
    assert O.loudness(short, 16000) == -math.inf                             # one sample short of a block
    lk, counts, _ = O.loudness(np.zeros(8000, np.float32), 16000, details=True)
    assert lk == -math.inf and counts == (2, 0, 0)


def _lib():
    import __graft_entry__ as g
    g.build()
    from knn_svc_amd import _lib
    return _lib.load()


def test_workspace_size_is_host_side():
    lib = _lib()
    sizes = [lib.knnsvc_loudness_workspace_bytes(n, 16000) for n in (0, 6399, 6400, 480000, 9600000)]
    assert all(s > 0 for s in sizes) and sizes == sorted(sizes), sizes
    assert lib.knnsvc_loudness_workspace_bytes(480000, 48000) > 0
    assert lib.knnsvc_loudness_workspace_bytes(480000, 11025) == 0 and b"sample rate" in lib.knnsvc_last_error()
    assert lib.knnsvc_loudness_workspace_bytes(-1, 16000) == 0 and b"length" in lib.knnsvc_last_error()


def test_layout_is_reported_by_the_library():
    """The GPU test takes its edge lengths from here, not from a copy of the kernel's constants."""
    from knn_svc_amd import ops
    _lib()
    chunk, group = ops.loudness_layout()
    assert chunk > 0 and group % chunk == 0 and group // chunk >= 64                 # whole chunks, at least one wave per workgroup
    assert chunk <= 800                                                              # no more than one step boundary per chunk at 8 kHz


def test_loudness_refuses_before_it_launches():
    """Dummy pointers, never dereferenced: every refusal below happens on the host, before the first launch."""
    lib = _lib()
    p = ctypes.c_void_p(256)
    rc = lib.knnsvc_loudness(p, 480000, 16000, p, None, p, 1, None)
    assert rc != 0 and b"workspace" in lib.knnsvc_last_error()
    big = lib.knnsvc_loudness_workspace_bytes(480000, 16000)
    assert lib.knnsvc_loudness(p, 480000, 11025, p, None, p, big, None) != 0 and b"sample rate" in lib.knnsvc_last_error()
    assert lib.knnsvc_loudness(p, -1, 16000, p, None, p, big, None) != 0 and b"length" in lib.knnsvc_last_error()
    assert lib.knnsvc_loudness(p, 480000, 16000, None, None, p, big, None) != 0 and b"null" in lib.knnsvc_last_error()
    assert lib.knnsvc_loudness_gain(p, 480000, None, -16.0, p, None) != 0 and b"null" in lib.knnsvc_last_error()
    assert lib.knnsvc_loudness_gain(p, 480000, p, float("nan"), p, None) != 0 and b"finite" in lib.knnsvc_last_error()


def test_ops_refuse_cpu_tensors():
    import torch
    from knn_svc_amd import ops
    from knn_svc_amd._lib import KnnSvcError
    with pytest.raises(KnnSvcError):
        ops.loudness(torch.zeros(8000))
    with pytest.raises(KnnSvcError):
        ops.normalize_loudness(torch.zeros(8000), -16.0)


def test_cli_switch():
    from knn_svc_amd.inference import build_parser
    a = build_parser().parse_args(["s", "t"])
    assert a.normalize_loudness is False and a.tgt_loudness_db == -16
    a = build_parser().parse_args(["s", "t", "--normalize_loudness", "true", "--tgt_loudness_db", "-20"])
    assert a.normalize_loudness is True and a.tgt_loudness_db == -20.0


def test_entry_points_carry_the_switch_off_by_default():
    from knn_svc_amd import ops, serving
    from knn_svc_amd.matcher import KNeighborsVC
    par = lambda fn: inspect.signature(fn).parameters
    assert par(KNeighborsVC.special_match)["normalize_loudness"].default is False
    assert par(KNeighborsVC.bulk_match)["normalize_loudness"].default is False
    assert par(KNeighborsVC.special_match)["tgt_loudness_db"].default == -16
    assert par(KNeighborsVC.bulk_match)["tgt_loudness_db"].default == -16
    assert par(KNeighborsVC.many_to_one)["loudness_db"].default is None
    assert par(serving.BatchConverter.__init__)["loudness_db"].default is None
    assert par(ops.loudness)["return_counts"].default is False and par(ops.loudness)["sample_rate"].default == 16000
    assert list(par(ops.normalize_loudness))[:2] == ["wav", "target_db"] and par(ops.normalize_loudness)["out"].default is None
