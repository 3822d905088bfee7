"""What the GPU tests that run their cases in a child interpreter share: the parent's runner, fixture and check, and the child's
report, case loop, comparisons and small-model fixtures.  A plain module (no conftest, no plugin); importing it neither initialises
the GPU nor imports knn_svc_amd.

To add such a test for a feature ``foo``:
  tests/foo_child.py       the docstring says what is asked and why; put the repository root on sys.path, then
                           ``from tests.gpu_child import note, same, ...``; write ``case_*`` functions that call
                           ``note(key, ok, detail)`` once per check (a case that takes a parameter is handed a temporary
                           directory); end with
                               if __name__ == "__main__":
                                   sys.exit(run_cases([("kernel", case_kernel), ("product", case_product)], sys.argv[1]))
                           run_cases notes ``<case>/ran`` and starts nothing more on the GPU after the first exception.
  tests/test_gpu_foo.py    ``pytestmark = pytest.mark.gpu``, a ``CHILD_TIMEOUT_S`` with a comment on how it was sized,
                               report = gpu_child.report_fixture("foo_child.py", "foo", CHILD_TIMEOUT_S)
                           tests that only read the report: ``gpu_child.check(report, "kernel/edges/", at_least=2)``; and
                           ``test_parent_process_left_the_gpu_alone``: the pytest process must not touch the GPU, because
                           test_gpu_dist2 spawns its ranks from it later."""
import contextlib
import inspect
import json
import os
import subprocess
import sys
import tempfile
import traceback

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda"
SENTINEL = -7.25e11
GUARD_ROWS = 64


# ------------------------------------------------------------------ parent side: never touches the GPU
def run_child(script, out_path, timeout_s, stdout_tail=12000) -> dict:
    """Run tests/<script> OUT_PATH in a fresh interpreter -> its report; ``__failed__`` says why when it timed out or exited
    with an error (next to whatever part of the report it wrote)."""
    try:
        r = subprocess.run([sys.executable, os.path.join("tests", script), out_path], timeout=timeout_s, cwd=ROOT,
                           capture_output=True, text=True)
    except subprocess.TimeoutExpired as e:
        return {"__failed__": f"child timed out after {timeout_s} s\n" + str(e.stderr or "")[-3000:]}
    print(r.stdout[-stdout_tail:])
    rep = {}
    if os.path.isfile(out_path):
        with open(out_path) as f:
            rep = json.load(f)
    if r.returncode != 0:
        rep["__failed__"] = f"child exited with {r.returncode}\n" + r.stderr[-3000:]
    return rep


def report_fixture(script, name, timeout_s, stdout_tail=12000):
    """The module-scoped ``report`` fixture of a parent: one child per module, started only from a process without a GPU."""
    import pytest

    @pytest.fixture(scope="module", name="report")
    def report(tmp_path_factory):
        if torch.cuda.is_initialized():
            pytest.skip("ranks are spawned from a process that has not initialised the GPU: run this module first / on its own")
        return run_child(script, str(tmp_path_factory.mktemp(name) / "report.json"), timeout_s, stdout_tail)
    return report


def check(report, prefix, at_least=None, exactly=None):
    """The child finished, wrote ``at_least`` (or ``exactly``) entries whose key starts with ``prefix``, and all of them are ok."""
    assert "__failed__" not in report, report["__failed__"]
    mine = {k: v for k, v in report.items() if k.startswith(prefix)}
    if exactly is not None:
        assert len(mine) == exactly, (prefix, sorted(mine))
    else:
        assert len(mine) >= at_least, (prefix, sorted(mine))
    bad = {k: v["detail"] for k, v in mine.items() if not v["ok"]}
    assert not bad, bad


# ------------------------------------------------------------------ child side: the report and the case loop
REPORT = {}


def note(name, ok, detail=""):
    REPORT[name] = {"ok": bool(ok), "detail": str(detail)}
    print(("ok   " if ok else "FAIL ") + name + (f"  [{detail}]" if detail else ""), flush=True)


def run_cases(cases, out_path, autograd=(), synchronize=None) -> int:
    """Run the (name, function) pairs in order and write the report -> the exit code.  A function that takes a parameter gets a
    temporary directory.  Every case runs under inference_mode unless its name is in ``autograd``.  ``synchronize`` is called
    after every case; None stands for the GPU: device 0 is selected and torch.cuda.synchronize used."""
    if synchronize is None:
        torch.cuda.set_device(0)
        synchronize = torch.cuda.synchronize
    rc = 0
    try:
        with tempfile.TemporaryDirectory() as tmp:
            for name, fn in cases:
                try:
                    with contextlib.nullcontext() if name in autograd else torch.inference_mode():
                        fn(tmp) if inspect.signature(fn).parameters else fn()
                    synchronize()
                except Exception:          # nothing more is started on the GPU after an error: report what ran and stop
                    note(f"{name}/ran", False, traceback.format_exc()[-1500:])
                    print(traceback.format_exc(), file=sys.stderr)
                    rc = 1
                    break
                note(f"{name}/ran", True)
    finally:
        with open(out_path, "w") as f:
            json.dump(REPORT, f, indent=1)
    return rc


# ------------------------------------------------------------------ child side: comparisons and operands
def same(a, b):
    """Bit equality of two tensors (or of two None): shapes and dtypes equal, float32 through the int32 view, so that NaN payloads
    and the sign of zero count.  The operands may live on different devices and need not be contiguous."""
    if a is None or b is None:
        return a is None and b is None
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    a, b = a.detach(), b.detach()
    if a.device != b.device:
        a, b = a.cpu(), b.cpu()
    if a.dtype == torch.float32:
        a, b = a.contiguous().view(torch.int32), b.contiguous().view(torch.int32)
    return torch.equal(a, b)


def x_equal(got, want):
    """A float32 tensor against a float32 numpy array -> (bit-identical?, number of differing elements; -1: shapes differ)"""
    got = got.cpu().numpy()
    if got.shape != want.shape:
        return False, -1
    bad = int((got.view(np.uint32) != want.view(np.uint32)).sum())
    return bad == 0, bad


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(DEV)


def table(lens):
    """Segment lengths -> the offsets table [0, l0, l0 + l1, ...]."""
    seg = [0]
    for n in lens:
        seg.append(seg[-1] + int(n))
    return seg


def misaligned(x_host):
    """The array on the device, contiguous, one float off a 16-byte boundary."""
    flat = torch.empty(x_host.size + 1, device=DEV, dtype=torch.float32)
    x = flat[1:].reshape(x_host.shape)
    x.copy_(dev(x_host))
    assert x.data_ptr() % 16 == 4 and x.is_contiguous()
    return x


def guarded(rows, *cols):
    """An output of ``rows`` rows with GUARD_ROWS rows of SENTINEL in front of and behind it -> (the output's view, a function
    that says whether every guard row still holds the sentinel)."""
    buf = torch.full((rows + 2 * GUARD_ROWS, *cols), SENTINEL, device=DEV)

    def untouched():
        return bool((buf[:GUARD_ROWS] == SENTINEL).all()) and bool((buf[GUARD_ROWS + rows:] == SENTINEL).all())
    return buf[GUARD_ROWS:GUARD_ROWS + rows], untouched


# ------------------------------------------------------------------ child side: product fixtures
def tiny_vc(kind="mix"):
    """The seeded small models (two encoder layers) behind a KNeighborsVC on the device."""
    from knn_svc_amd import config as C, synthetic as S
    from knn_svc_amd.matcher import KNeighborsVC
    from knn_svc_amd.vocoder import Vocoder
    from knn_svc_amd.wavlm import WavLMEncoder
    cfg, h = C.WAVLM_TINY, C.HIFIGAN_TINY
    enc = WavLMEncoder(S.seeded_state(S.wavlm_param_spec(cfg), seed=11), cfg, DEV, n_layers=2)
    return KNeighborsVC(enc, Vocoder(S.seeded_state(S.generator_param_spec(h, kind), 63 if kind == "mix" else 64), h, kind, DEV), h, DEV)


def write_clip(path, n, seed, f0=None, f0_mul=1.0, gain=None):
    """Write the seeded synthetic clip of ``n`` samples as PCM16 to ``path`` (.wav), times ``gain`` (an array) where given, and
    its f0 track next to it: ``f0`` as it is where given, else the clip's own track times ``f0_mul``."""
    from knn_svc_amd import audio_io, synthetic as S
    w, f = S.synth_clip(n, seed=seed)
    if gain is not None:
        w = (w * gain).astype(np.float32)
    audio_io.write_wav_pcm16(path, w, 16000)
    np.save(path[:-4] + "_f0.npy", f0 if f0 is not None else (f * f0_mul).astype(np.float32))
