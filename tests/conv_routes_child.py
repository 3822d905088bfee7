"""Child interpreter of tests/test_gpu_conv_routes.py: launches every row of the route table (tests/conv_routes_common.py) on
the GPU and writes what it measured as JSON; the pytest process reads the report and asserts on it (it sorts in front of
test_gpu_dist2 and must not initialise the GPU itself).

    python tests/conv_routes_child.py REPORT.json

Nothing is judged here: a record holds the kernel and epilogue the dispatcher reported, per descriptor the error against fp64,
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


class _Knobs:
    """The row's dispatcher knobs and weight split in the environment for the length of a `with`, then what was there before."""

    def __init__(self, case):
        self.env = dict(case.env)
        if case.split:
            self.env["KNNSVC_GEMM"] = case.split

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.env}
        os.environ.update(self.env)
        _ops().reload_knobs()

    def __exit__(self, *exc):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
        _ops().reload_knobs()


class _Launch:
    """One descriptor of a row on the device: operands, the sentinel-framed output buffer and the conv_gemm call."""

    def __init__(self, case, inp, rows_alloc=None, x_rows_alloc=None):
        ops = _ops()
        self.case, c = case, case
        B, G = c.batches, c.groups
        self.rows_alloc = rows_alloc or c.rows                      # a bucketed launch is laid out for more rows than are valid
        x = inp["x"]
        if x_rows_alloc:                                            # rows behind the valid input: finite junk the kernel must not read
            x = torch.cat([x, torch.full((B, x_rows_alloc - x.shape[1], x.shape[2]), 7.0)], 1)
        self.t_alloc = x.shape[1]
        x2d = x.reshape(-1, G * c.cin)
        self.x = (ops.split_pack(x2d) if c.x_split else x2d.contiguous()).to(DEV)
        if c.convt:
            wp = ops.pack_convT_weight(inp["w"], c.convt[0])
        elif G > 1:
            wp = ops.pack_grouped_conv_weight(inp["w"], G)
        else:
            wp = ops.pack_conv_weight(inp["w"])
        self.w = wp.to(DEV)
        if c.split:
            self.w = ops.attach_split(self.w)
            assert hasattr(self.w, "_w3" if c.split == "bf16x3" else "_w2"), "the weights did not take the split this row is about"
        self.bias = inp["bias"].to(DEV) if inp["bias"] is not None else None
        self.resid = None
        if inp["resid"] is not None:
            r = torch.zeros(B, c.rows, c.ldr)
            r[:, :, :c.width] = inp["resid"]
            self.resid = r.to(DEV)
        self.prev = inp["prev"]
        self.pitch = self.rows_alloc + R.ROW_GAP                    # rows from one batch item's block to the next
        self.buf = torch.empty(R.ROW_GAP + B * self.pitch, c.ldo, device=DEV)
        self.slot = ops.new_slot(DEV) if c.slot else None
        self.reset()

    def reset(self):
        c = self.case
        self.buf.fill_(R.SENTINEL)
        if self.prev is not None:
            self._blocks()[:, :c.rows, :c.width] = self.prev.to(DEV)
        if self.slot is not None:
            self.slot.zero_()

    def _blocks(self):
        return self.buf[R.ROW_GAP:].view(self.case.batches, self.pitch, self.case.ldo)

    def valid(self, rows=None):
        return self._blocks()[:, :rows or self.case.rows, :self.case.width]

    def outside_is_untouched(self, rows=None):
        """Every float outside the [rows, width] blocks still holds the sentinel's bits."""
        mask = torch.ones_like(self.buf, dtype=torch.bool)
        mask[R.ROW_GAP:].view(self.case.batches, self.pitch, self.case.ldo)[:, :rows or self.case.rows, :self.case.width] = False
        return bool((self.buf[mask] == R.SENTINEL).all()), int((self.buf[mask] != R.SENTINEL).sum())

    def launch(self, defer=None, dyn=None):
        ops, c = _ops(), self.case
        B, G = c.batches, c.groups
        ldx = G * c.cin
        kw = dict(m=c.m if dyn is None else self._m_alloc, n=c.n, cin=c.cin, taps=c.k, stride=c.stride, dil=c.dil, pad=c.pad_,
                  t_in=self.t_alloc if dyn is not None else c.t_in_, ldx=ldx, ldo=c.ldo, bias=self.bias, a_slope=c.a_slope, act=c.act,
                  act_slope=c.act_slope, accumulate=c.accumulate, div=c.div, batches=B, groups=G, x_bstride=self.t_alloc * ldx,
                  o_bstride=self.pitch * c.ldo, x_split=c.x_split, out_absmax=self.slot, defer=defer, dyn=dyn)
        if G > 1:
            kw.update(x_gstride=c.cin, w_gstride=c.n * c.cin * c.k, bias_gstride=c.n, o_gstride=c.n, r_gstride=c.n)
        if self.resid is not None:
            kw.update(resid=self.resid, ldr=c.ldr, r_bstride=c.rows * c.ldr)
        if c.convt:
            u, cout = c.convt
            kw.update(bias_period=cout if self.bias is not None else 0, convt_u=u, convt_cout=cout, convt_pad=(c.k * u - u) // 2,
                      t_out=self.rows_alloc)
        ops.conv_gemm(self.x, self.w, self.buf[R.ROW_GAP:], **kw)

    def launch_bucket(self, bucket_case, dyn):
        """This (exact-length) descriptor's data through a launch laid out for `bucket_case`'s lengths."""
        self._m_alloc = bucket_case.m
        self.launch(dyn=dyn)


def _same_bits(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


def run_row(case) -> dict:
    """Launch a row twice -> its record."""
    ops = _ops()
    with _Knobs(case):
        ls = [_Launch(d, R.prepared(d)[0]) for d in case.descs()]

        def go():
            for l in ls:
                l.reset()
            if case.branches:
                descs = []
                for l in ls:
                    l.launch(defer=descs)
                ops.conv_gemm_multi(descs)
            else:
                ls[0].launch()
            torch.cuda.synchronize()
            return ops.last_conv_kernel(), ops.last_conv_epilogue()
        tag, epi = go()
        first = [(l.buf.clone(), l.slot.clone() if l.slot is not None else None) for l in ls]
        rec = dict(tag=tag, epi=epi, descs=[])
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
    with _Knobs(bucket_case):
        inp, ref64, e32, scale = R.prepared(exact_case)
        exact = _Launch(exact_case, inp)
        exact.launch()
        torch.cuda.synchronize()
        rec = dict(exact_tag=ops.last_conv_kernel(), err=float((exact.valid().cpu().double() - ref64).abs().max()), e32=e32, scale=scale)
        bl = _Launch(exact_case, inp, rows_alloc=bucket_case.rows, x_rows_alloc=bucket_case.t_in_)
        nd = torch.tensor([count], device=DEV, dtype=torch.int32)
        bl.launch_bucket(bucket_case, (nd, bucket))
        torch.cuda.synchronize()
        rec.update(tag=ops.last_conv_kernel(), epi=ops.last_conv_epilogue(), same_bits=_same_bits(bl.valid(), exact.valid()),
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
