"""CPU: tests/gpu_child.py itself — the runner and the check of the parents, the case loop, the comparisons and the clip writer of
the children.  No GPU: the fake children are tiny scripts that import neither torch nor the project, and the case loop runs with
a synchronise that does nothing."""
import json
import time

import numpy as np
import pytest
import torch

from tests import blend_oracle, gpu_child as G

ENTRY = {"ok": True, "detail": ""}


def _script(tmp_path, body):
    p = tmp_path / "fake_child.py"
    p.write_text("import json, sys, time\n" + body)
    return str(p)


# ------------------------------------------------------------------ run_child
def test_run_child_returns_the_report_as_written(tmp_path, capsys):
    s = _script(tmp_path, "print('hello from the child')\njson.dump({'a/x': {'ok': True, 'detail': 'd'}}, open(sys.argv[1], 'w'))\n")
    assert G.run_child(s, str(tmp_path / "r.json"), 60) == {"a/x": {"ok": True, "detail": "d"}}
    assert "hello from the child" in capsys.readouterr().out


def test_run_child_keeps_a_partial_report_next_to_the_failure(tmp_path):
    s = _script(tmp_path, "json.dump({'a/x': {'ok': True, 'detail': ''}}, open(sys.argv[1], 'w'))\n"
                          "print('the reason', file=sys.stderr)\nsys.exit(1)\n")
    rep = G.run_child(s, str(tmp_path / "r.json"), 60)
    assert set(rep) == {"a/x", "__failed__"} and rep["a/x"] == ENTRY
    assert rep["__failed__"].startswith("child exited with 1\n") and "the reason" in rep["__failed__"]


def test_run_child_without_a_report_has_only_the_failure(tmp_path):
    rep = G.run_child(_script(tmp_path, "sys.exit(3)\n"), str(tmp_path / "r.json"), 60)
    assert set(rep) == {"__failed__"} and rep["__failed__"].startswith("child exited with 3\n")


def test_run_child_ends_a_child_that_outlives_its_timeout(tmp_path):
    t0 = time.monotonic()
    rep = G.run_child(_script(tmp_path, "time.sleep(30)\n"), str(tmp_path / "r.json"), 1)
    assert time.monotonic() - t0 < 30
    assert set(rep) == {"__failed__"} and rep["__failed__"].startswith("child timed out after 1 s\n")


# ------------------------------------------------------------------ check
def test_check_passes_at_the_bar():
    rep = {"a/1": ENTRY, "a/2": ENTRY, "b/1": {"ok": False, "detail": "not mine"}}
    G.check(rep, "a/", 2)
    G.check(rep, "a/", at_least=1)
    G.check(rep, "a/", exactly=2)


def test_check_fails_with_too_few_keys():
    with pytest.raises(AssertionError, match="a/1"):
        G.check({"a/1": ENTRY}, "a/", 2)


def test_check_fails_on_an_exactly_mismatch():
    with pytest.raises(AssertionError):
        G.check({"a/1": ENTRY, "a/2": ENTRY}, "a/", exactly=1)
    with pytest.raises(AssertionError):
        G.check({"a/1": ENTRY, "a/2": ENTRY}, "a/", exactly=3)


def test_check_fails_on_one_entry_that_is_not_ok_and_shows_its_detail():
    with pytest.raises(AssertionError, match="3 elements differ"):
        G.check({"a/1": ENTRY, "a/2": {"ok": False, "detail": "3 elements differ"}}, "a/", 2)


def test_check_fails_on_a_failed_child_whatever_it_reported():
    with pytest.raises(AssertionError, match="child exited with 1"):
        G.check({"a/1": ENTRY, "__failed__": "child exited with 1\n"}, "a/", 1)


# ------------------------------------------------------------------ run_cases
@pytest.fixture
def empty_report():
    G.REPORT.clear()
    yield G.REPORT
    G.REPORT.clear()


def test_run_cases_stops_at_the_first_exception(tmp_path, empty_report):
    ran, synced = [], []

    def first():
        ran.append("first")
        G.note("first/a", True, "fine")

    def second():
        ran.append("second")
        G.note("second/a", True)
        raise RuntimeError("the kernel failed")

    def third():
        ran.append("third")
    out = tmp_path / "r.json"
    rc = G.run_cases([("first", first), ("second", second), ("third", third)], str(out), synchronize=lambda: synced.append(1))
    rep = json.loads(out.read_text())
    assert rc == 1 and ran == ["first", "second"] and synced == [1]
    assert rep["first/a"] == {"ok": True, "detail": "fine"} and rep["first/ran"] == ENTRY and rep["second/a"] == ENTRY
    assert rep["second/ran"]["ok"] is False
    assert "Traceback" in rep["second/ran"]["detail"] and "RuntimeError: the kernel failed" in rep["second/ran"]["detail"]
    assert not [k for k in rep if k.startswith("third")]


def test_run_cases_returns_zero_when_every_case_passes(tmp_path, empty_report):
    seen = []

    def wants_a_directory(tmp):
        seen.append(tmp)
        (tmp_path / "probe").write_text(str(__import__("os").path.isdir(tmp)))
    out = tmp_path / "r.json"
    assert G.run_cases([("a", lambda: None), ("b", wants_a_directory)], str(out), synchronize=lambda: None) == 0
    assert json.loads(out.read_text()) == {"a/ran": ENTRY, "b/ran": ENTRY}
    assert len(seen) == 1 and (tmp_path / "probe").read_text() == "True"


def test_run_cases_gives_autograd_only_to_the_cases_that_ask(tmp_path, empty_report):
    modes = {}

    def look(name):
        return lambda: modes.__setitem__(name, (torch.is_grad_enabled(), torch.is_inference_mode_enabled()))
    rc = G.run_cases([("plain", look("plain")), ("adam", look("adam")), ("after", look("after"))], str(tmp_path / "r.json"),
                     autograd=("adam",), synchronize=lambda: None)
    assert rc == 0 and modes == {"plain": (False, True), "adam": (True, False), "after": (False, True)}


# ------------------------------------------------------------------ same, table, x_equal
def test_same_is_bit_equality():
    nan = torch.tensor([0x7FC00001, 0x7FC00000], dtype=torch.int32).view(torch.float32)
    assert G.same(nan, nan.clone())                                                     # equal NaN bit patterns
    assert not G.same(nan, nan.flip(0))                                                 # NaN payloads count
    assert not G.same(torch.tensor([0.0]), torch.tensor([-0.0]))
    assert not G.same(torch.zeros(3), torch.zeros(3, dtype=torch.float64))
    assert not G.same(torch.zeros(3, dtype=torch.int32), torch.zeros(3, dtype=torch.int64))
    assert not G.same(torch.zeros(3), torch.zeros(3, 1))
    assert G.same(None, None)
    assert not G.same(None, torch.zeros(1)) and not G.same(torch.zeros(1), None)
    x = torch.arange(24, dtype=torch.float32).reshape(4, 6)
    assert not x.t().is_contiguous() and G.same(x.t(), x.t().contiguous()) and G.same(x[:, ::2], x[:, ::2].clone())
    assert not G.same(x.t(), x.reshape(6, 4))
    assert G.same(torch.arange(5), torch.arange(5)) and not G.same(torch.arange(5), torch.arange(5).flip(0))


def test_table_and_x_equal():
    assert G.table([1, 2, 5]) == [0, 1, 3, 8] and G.table([]) == [0]
    want = np.array([[1.0, -0.0, 3.0], [4.0, 5.0, np.nan]], np.float32)
    assert G.x_equal(torch.from_numpy(want.copy()), want) == (True, 0)
    got = want.copy()
    got[0, 1], got[1, 0] = 0.0, 4.5                                                     # the sign of a zero, and a value
    assert G.x_equal(torch.from_numpy(got), want) == (False, 2)
    assert G.x_equal(torch.from_numpy(want[:1].copy()), want) == (False, -1)


# ------------------------------------------------------------------ write_clip
def _bytes(path):
    with open(path, "rb") as f:
        return f.read()


def test_write_clip_writes_the_bytes_of_the_statements_it_replaces(tmp_path):
    from knn_svc_amd import audio_io, synthetic as S
    n, seed = 9000, 703
    a, b = str(tmp_path / "a.wav"), str(tmp_path / "b.wav")

    def equal():
        return _bytes(a) == _bytes(b) and _bytes(a[:-4] + "_f0.npy") == _bytes(b[:-4] + "_f0.npy")
    # the clip's own track, as it is (a pool) and times 1.2 (a source)
    for mul in (1.0, 1.2):
        w, f = S.synth_clip(n, seed=seed)
        audio_io.write_wav_pcm16(a, w, 16000)
        np.save(a[:-4] + "_f0.npy", f if mul == 1.0 else f * mul)
        G.write_clip(b, n, seed, f0_mul=mul)
        assert equal(), mul
    # a track from an oracle
    w, _f = S.synth_clip(n, seed=seed)
    audio_io.write_wav_pcm16(a, w, 16000)
    np.save(a[:-4] + "_f0.npy", blend_oracle.track(len(w) // 320 + 1, 233.0, 40))
    G.write_clip(b, n, seed, f0=blend_oracle.track(n // 320 + 1, 233.0, 40))
    assert equal()
    # a phrased gain on the waveform
    gain = np.repeat(np.random.default_rng(5).uniform(0.0, 1.0, 9), 1000)
    w, f = S.synth_clip(n, seed=seed)
    w = (w * gain).astype(np.float32)
    audio_io.write_wav_pcm16(a, w, 16000)
    np.save(a[:-4] + "_f0.npy", (f * 1.25).astype(np.float32))
    G.write_clip(b, n, seed, f0_mul=1.25, gain=gain)
    assert equal()
