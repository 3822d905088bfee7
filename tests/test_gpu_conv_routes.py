"""GPU: every kernel knnsvc_conv_gemm can dispatch to, reached by name and held to an fp64 reference.

The rows, the references and the tolerance are in tests/conv_routes_common.py.  All GPU work runs in ONE fresh child interpreter
(tests/conv_routes_child.py) that writes what it measured; the tests here read that report and judge it.  This module sorts in
front of test_gpu_dist2, which must find the interpreter without an initialised GPU, so nothing here touches the GPU in the pytest
process — unless something else already has: then the same rows run in this process, no child is started and nothing is skipped.
Per row:
  route         ops.last_conv_kernel() (and last_conv_epilogue() where the row names one) is what the row expects; a row that lands
                on another kernel FAILS — it is not skipped; and it is what ops.conv_route answered before the launch;
  accuracy      max |out - ref64| <= F * e32 + 1e-6 * max |ref64|, e32 = max |torch fp32 on the CPU - ref64| on the same inputs, one
                F per family of kernels;
  stray stores  the output lies in a sentinel-filled buffer: ROW_GAP rows in front of and behind every batch item, COL_SLACK
                columns behind every row; everything outside the [rows, width] blocks is bit-unchanged afterwards;
  range slot    f16x2 rows that pass out_absmax: the slot's maximum is max |out| over the valid blocks, exactly;
  determinism   a second launch gives the same bits.

Measured on an MI355X, err / e32 per row (the worst descriptor of a merged grid); e32 was 1.6e-7 .. 5.2e-6 there:

  f16x2   W128D 0.92  W128S 1.17  W128 1.12  W160 1.11  W64 1.32  W32 1.37  W64P 0.87  W64P-grouped 0.75
          F64S 0.58  F128 0.87  F64 0.62  F32 1.27  W128Dx 1.22  W128Sx 1.23  W128x 1.04  W160x 1.30  W64x 0.79  W32x 1.19
          W64Px 0.99  F128a2 0.85  F64-a2 0.68  F32-a2 0.67  Q256S 1.74  Q256S-gelu 2.00  Q256S-resid-slot 2.45
          F128-convt 0.73  F64S-convt 1.08  F64-convt 0.99  F32-convt 1.17  W128D-generic-epilogue 1.18  F64-win-off 1.29
          W128D-one-row 1.33  W64-shorter-than-halo 0.83  W128D-resid-other-pitch 0.97                          worst 2.45
  bf16x3  H128 1.24  H64 1.24  H32 1.52                                                                        worst 1.52
  fp32    G128v8 1.47  G64v8 0.77  G32v8 1.62  G128v4 1.78  G64v4 1.50  G32v4 1.29  G128v1-cin34 2.17  G64v1-cin1 0.68
          G32v1-cin34 1.56  G128v1-cin1 0.88  G64v1-cin34 1.72  G32v1-cin1 0.95                                 worst 2.17

F of a family is twice its worst ratio, rounded up: 5 / 4 / 5, under the cap of 16.  For scale: a dropped low-half product of the
f16x2 split is 450 .. 1000 x e32, a misplaced row or tap >= 1e4 x e32; a ratio above 8 on any row is a finding, not a bar to raise.
Every row kept all five properties in that run but one: W64-shorter-than-halo (m = 7 of a 256-row tile) found rows past M — which
the lean epilogues compute and leave to the buffer range check — in the range slot (3.6204 against max |out| = 3.5084); the
epilogues now leave them out (row_keep in conv_gemm.hip).
"""
import pytest
import torch

from tests import conv_routes_common as R, gpu_child

pytestmark = pytest.mark.gpu
CHILD_TIMEOUT_S = 300        # measured: 15 s for the child on a warm machine, 9 s of it the references on the CPU; the rest is for a cold torch import

# F per family = twice the worst err / e32 measured over the table on an MI355X, rounded up (cap 16: see the table above)
FACTOR = {"fp32": 5, "bf16x3": 4, "f16x2": 5}
assert all(f <= 16 for f in FACTOR.values())


@pytest.fixture(autouse=True)
def _knobs_back_to_default(monkeypatch):
    yield
    monkeypatch.undo()
    if torch.cuda.is_initialized():          # (rows ran in this process: have the library read the restored environment)
        from knn_svc_amd import ops
        ops.reload_knobs()


@pytest.fixture(scope="module")
def report(tmp_path_factory):
    if torch.cuda.is_initialized():
        from tests import conv_routes_child
        return conv_routes_child.run_all(print)
    return gpu_child.run_child("conv_routes_child.py", str(tmp_path_factory.mktemp("conv_routes") / "report.json"), CHILD_TIMEOUT_S)


def _record(report, id_):
    assert "__failed__" not in report, report["__failed__"]
    assert id_ in report, f"{id_}: the row did not run"
    return report[id_]


@pytest.mark.parametrize("case", R.CASES, ids=lambda c: c.id)
def test_route_against_fp64(case, report):
    rec = _record(report, case.id)
    tag, epi = rec["tag"], rec["epi"]
    assert tag == case.tag, f"{case.id}: dispatched to {tag}, the row is about {case.tag}"
    if case.epi is not None:
        assert epi == case.epi, f"{case.id}: epilogue {epi!r}, expected {case.epi!r}"
    assert rec["route"] == [tag, epi], f"{case.id}: the route entry answered {rec['route']}, the launch took {tag}/{epi}"
    assert len(rec["descs"]) == len(case.descs())
    for d in rec["descs"]:
        err, e32 = d["err"], d["e32"]
        tol = R.tolerance(FACTOR[case.family], e32, d["scale"])
        print(f"{case.id} k={d['k']}: {tag}/{epi} err {err:.3e} e32 {e32:.3e} ratio {err / e32:.2f} (tolerance {tol:.3e})")
        assert err <= tol, f"{case.id} k={d['k']}: err {err:.3e} = {err / e32:.1f} x e32, tolerance {tol:.3e}"
        assert d["stray"] == 0, f"{case.id} k={d['k']}: {d['stray']} floats outside the output blocks were written"
        if case.slot and case.family == "f16x2":
            assert d["slot"] is not None and d["slot"][0] == d["slot"][1], (case.id, d["slot"])
    assert rec["same_bits_again"], f"{case.id}: a second launch gives other bits"


@pytest.mark.parametrize("row", R.DYN_CASES, ids=lambda r: r[0].id)
def test_bucketed_launch_equals_exact_length(row, report):
    """dyn = (count, bucket), count < bucket: the launch laid out for the bucket writes, on the count's rows, the bits of the
    exact-length launch, and leaves the rows behind them alone (the input rows behind the valid ones hold junk)."""
    bucket_case = row[0]
    rec = _record(report, bucket_case.id)
    assert rec["exact_tag"] == bucket_case.tag == rec["exact_route"]
    assert rec["err"] <= R.tolerance(FACTOR[bucket_case.family], rec["e32"], rec["scale"]), (rec["err"], rec["e32"])
    assert (rec["tag"], rec["epi"]) == (bucket_case.tag, bucket_case.epi) == tuple(rec["route"])
    assert rec["same_bits"]
    assert rec["stray"] == 0, f"{rec['stray']} floats behind the valid rows or outside the blocks were written"
    assert rec["slots"][0] == rec["slots"][1] == rec["slots"][2], rec["slots"]
