"""Child interpreter of tests/test_gpu_conv_routes.py: launches every row of the route table (tests/conv_routes_common.py) on
the GPU and writes what it measured as JSON; the pytest process reads the report and asserts on it (it sorts in front of
test_gpu_dist2 and must not initialise the GPU itself).

    python tests/conv_routes_child.py REPORT.json

Nothing is judged here: a record holds the kernel and epilogue the dispatcher reported after the launch and what its route entry
(ops.conv_route) answered to the same descriptors before it, per descriptor the error against fp64,
e32 and the output's scale, the number of floats written outside the output blocks, the range slot next to max |out|, and whether
a second launch gave the same bits.  The first error that is not a measurement (a failed launch) ends the run."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch

from tests import conv_routes_common as R

DEV = "cuda"


def _ops():
    from knn_svc_amd import ops
    return ops


def _same_bits(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


def run_row(case) -> dict:
    """Launch a row twice -> its record."""
    ops = _ops()
    with R.Knobs(case):
        ls = [R.Launch(d, R.prepared(d)[0]) for d in case.descs()]

        def go():
            for l in ls:
                l.reset()
            descs = []
            for l in ls:
                l.launch(defer=descs)
            asked = ops.conv_route(descs)                           # what the dispatcher says it will do, before it does it
            if case.branches:
                ops.conv_gemm_multi(descs)
            else:
                ls[0].launch()
            torch.cuda.synchronize()
            return ops.last_conv_kernel(), ops.last_conv_epilogue(), asked
        tag, epi, asked = go()
        first = [(l.buf.clone(), l.slot.clone() if l.slot is not None else None) for l in ls]
        rec = dict(tag=tag, epi=epi, route=list(asked), descs=[])
        for l in ls:
            _, ref64, e32, scale = R.prepared(l.case)
            out = l.valid().cpu()
            rec["descs"].append(dict(k=l.case.k, err=float((out.double() - ref64).abs().max()), e32=e32, scale=scale,
                                     stray=l.outside_is_untouched()[1],
                                     slot=None if l.slot is None else [float(l.slot.max()), float(out.abs().max())]))
        go()
        rec["same_bits_again"] = all(_same_bits(l.buf, buf) and (slot is None or torch.equal(l.slot, slot)) for l, (buf, slot) in zip(ls, first))
    return rec


def run_dyn(row) -> dict:
    """The exact-length launch and the bucketed one (dyn = (count, bucket), junk in the input rows behind the valid ones) -> record."""
    ops = _ops()
    bucket_case, per, count, bucket = row
    exact_case = R.dyn_exact(bucket_case, per, count, bucket)
    with R.Knobs(bucket_case):
        inp, ref64, e32, scale = R.prepared(exact_case)
        exact = R.Launch(exact_case, inp)
        exact_route = exact.route()
        exact.launch()
        torch.cuda.synchronize()
        rec = dict(exact_tag=ops.last_conv_kernel(), exact_route=exact_route[0], err=float((exact.valid().cpu().double() - ref64).abs().max()), e32=e32, scale=scale)
        bl = R.Launch(exact_case, inp, rows_alloc=bucket_case.rows, x_rows_alloc=bucket_case.t_in_)
        nd = torch.tensor([count], device=DEV, dtype=torch.int32)
        dyn = dict(dyn=(nd, bucket), m_alloc=bucket_case.m)         # this descriptor's data, laid out for the bucket's lengths
        route = bl.route(**dyn)
        bl.launch(**dyn)
        torch.cuda.synchronize()
        rec.update(route=list(route), tag=ops.last_conv_kernel(), epi=ops.last_conv_epilogue(), same_bits=_same_bits(bl.valid(), exact.valid()),
                   stray=bl.outside_is_untouched()[1],
                   slots=[float(bl.slot.max()), float(exact.slot.max()), float(exact.valid().abs().max())])
    return rec


def run_all(say=lambda *a: None) -> dict:
    report = {}
    for case in R.CASES:
        report[case.id] = rec = run_row(case)
        for d in rec["descs"]:
            say(f"{case.id} k={d['k']}: {rec['tag']}/{rec['epi']} err {d['err']:.3e} e32 {d['e32']:.3e} ratio {d['err'] / d['e32']:.2f} "
                f"stray {d['stray']} slot {d['slot']} again {rec['same_bits_again']}")
    for row in R.DYN_CASES:
        report[row[0].id] = rec = run_dyn(row)
        say(f"{row[0].id}: {rec}")
    return report


if __name__ == "__main__":
    rep = run_all(lambda *a: print(*a, flush=True))
    with open(sys.argv[1], "w") as f:
        json.dump(rep, f)
