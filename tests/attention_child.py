"""Child interpreter of tests/test_gpu_attention.py: launches the rows of tests/attention_oracle.py on the GPU and notes what it
measured; the pytest process reads the report and judges it (it must not initialise the GPU itself).

    python tests/attention_child.py REPORT.json            every row but those of the fp32 route
    python tests/attention_fp32_child.py REPORT.json       KNNSVC_ATTENTION=fp32 (the library reads it once per process)

Nothing is judged here: every note is `ok` and carries a JSON record in its detail —
  row/<id>       the tag the dispatcher reported, err = max |out - ref64| over the query rows below kv_len, e32 and scale from the
                 oracle, max |ref64|, whether every output row is finite, whether the guard rows around the output still hold the
                 sentinel, whether a second launch gave the same bits, and (f16x2 rows) per schedule the shape admits the tag it
                 reported and whether it gave the same bits;
  bucket/<id>/n  rows < n of a launch at T with kv_len = n against a launch at exactly n frames (table columns [T-n, T+n-1)): same bits?
  batch/<id>     a B = 3 launch against three B = 1 launches: same bits?
  refuse/<id>    the return code and message of a call that must be refused, whether the last-kernel tag and the output moved;
  route/asked    how many launches there were, and those whose tag was not what ops.attention_route had answered just before.
The first exception ends the run (gpu_child.run_cases)."""
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch

from tests import attention_oracle as A
from tests.gpu_child import DEV, guarded, misaligned, note, run_cases, same

KNOBS = ("KNNSVC_ATT_QB", "KNNSVC_ATT_NW")
FP32 = os.environ.get("KNNSVC_ATTENTION", "")[:2] == "fp"       # set by attention_fp32_child.py before this module is imported


def _ops():
    from knn_svc_amd import ops
    return ops


def _lib():
    from knn_svc_amd import _lib
    return _lib.load()


def set_knobs(env):
    """The dispatcher's per-call knobs as the row wants them, every other one unset."""
    for k in KNOBS:
        os.environ.pop(k, None)
    os.environ.update({k: v for k, v in env if k in KNOBS})


def _ptr(t):
    return ctypes.c_void_p(0 if t is None else t.data_ptr())


def raw(qkv, gate, table, B, T, H, out, flags=0, kv_split=0, kv_len=None):
    """knnsvc_wavlm_attention as it is -> (return code, message)."""
    rc = _lib().knnsvc_wavlm_attention(_ptr(qkv), _ptr(gate), _ptr(table), B, T, H, _ptr(out), flags, kv_split, _ptr(kv_len),
                                       ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    return rc, _lib().knnsvc_last_error().decode("utf-8", "replace") if rc else ""


ROUTES = [0, []]          # launches, and those that took another kernel than the route entry had answered


class Operands:
    """q, k, v, gate, table of the oracle on the device, as the kernel takes them."""

    def __init__(self, q, k, v, gate, table, kv_len=None, kv_split=False):
        B, T, H, _ = q.shape
        self.B, self.T, self.H, self.E = B, T, H, H * A.HD
        flat = lambda x: x.reshape(B * T, self.E)
        kk, vv = flat(k), flat(v)
        if kv_split:
            kk, vv = _ops().split_pack(kk), _ops().split_pack(vv)
        self.qkv = torch.cat([flat(q), kk, vv], 1).contiguous().to(DEV)
        self.gate = gate.reshape(B * T, H).contiguous().to(DEV)
        self.table = table.contiguous().to(DEV)
        self.kv_len = None if kv_len is None else torch.tensor(kv_len, dtype=torch.int32, device=DEV)
        self.kv_split = kv_split

    def launch(self, wide=False, out_split=False):
        """-> (output [B*T, E] inside guard rows (unpacked where split), guard check, tag)"""
        out, untouched = guarded(self.B * self.T, self.E)
        asked = _ops().attention_route(self.B, self.T, self.H, out_split, self.kv_split, wide)[0]
        rc, msg = raw(self.qkv, self.gate, self.table, self.B, self.T, self.H, out, (1 if out_split else 0) | (4 if wide else 0),
                      1 if self.kv_split else 0, self.kv_len)
        if rc:
            raise RuntimeError(f"wavlm_attention failed ({rc}): {msg}")
        torch.cuda.synchronize()
        tag = _ops().last_attention_kernel()
        ROUTES[0] += 1
        if asked != tag:
            ROUTES[1].append(f"B {self.B} T {self.T} H {self.H}: asked {asked}, launched {tag}")
        return out, untouched, tag


def run_row(case) -> dict:
    q, k, v, gate, table = A.inputs(case)
    ref, e32, scale, valid = A.yardstick(case)
    op = Operands(q, k, v, gate, table, case.kv_len, case.kv_split)
    set_knobs(case.env)
    out, untouched, tag = op.launch(case.wide, case.out_split)
    val = (_ops().split_unpack(out) if case.out_split else out).cpu().view(case.B, case.T, case.H, A.HD)
    d = (val[:, case.rows()].double() - ref).abs()
    rec = dict(tag=tag, err=float(d[valid].max()), e32=e32, scale=scale, omax=float(ref[valid].abs().max()),
               finite=bool(torch.isfinite(val).all()), guard=untouched())
    again, _, _ = op.launch(case.wide, case.out_split)
    rec["again"] = same(again, out)
    if case.route == "f16x2":
        rec["sched"] = {}
        for env, want in A.schedules(case.T):
            set_knobs(env)
            other, _, got = op.launch(False, case.out_split)
            rec["sched"][want] = [got, same(other, out)]
    set_knobs(())
    return rec


def _mine(tag):
    return (tag == A.TAG_F32) == FP32


def case_rows():
    for case in A.CASES:
        if case.fp32_child == FP32:
            rec = run_row(case)
            note(f"row/{case.id}", True, json.dumps(rec))


def case_bucket():
    for id_, tag, T, H, env, wide in A.BUCKETS:
        if not _mine(tag):
            continue
        q, k, v, gate, table = A.family_inputs("model", 1, T, H, seed=5)
        for n in A.BUCKET_N:
            jq, jk, jv = (x.clone() for x in (q, k, v))
            for x in (jq, jk, jv):
                x[:, n:] = A.JUNK
            set_knobs(env)
            big, _, tag_big = Operands(jq, jk, jv, gate, table, (n,)).launch(wide)
            exact, untouched, tag_exact = Operands(q[:, :n], k[:, :n], v[:, :n], gate[:, :n], A.bucket_table(table, T, n)).launch(wide)
            note(f"bucket/{id_}/{n}", True, json.dumps(dict(tag=tag_big, tag_exact=tag_exact, same=same(big[:n], exact), guard=untouched())))
    set_knobs(())


def case_batch():
    for id_, tag, T, H, kv_len, env, wide in A.BATCHES:
        if not _mine(tag):
            continue
        q, k, v, gate, table = A.family_inputs("model", 3, T, H, seed=6)
        set_knobs(env)
        all3, _, tag3 = Operands(q, k, v, gate, table, kv_len).launch(wide)
        ones = [Operands(q[b:b + 1], k[b:b + 1], v[b:b + 1], gate[b:b + 1], table, kv_len[b:b + 1]).launch(wide) for b in range(3)]
        note(f"batch/{id_}", True, json.dumps(dict(tag=tag3, tags=[o[2] for o in ones], same=same(all3, torch.cat([o[0] for o in ones])))))
    set_knobs(())


def _refusal(id_, before, call):
    """`call(out)` must be refused: note its code and message, and whether the tag or the output moved."""
    out, _ = guarded(4 * 8, 2 * A.HD)
    out.fill_(-3.0)
    rc, msg = call(out)
    torch.cuda.synchronize()
    note(f"refuse/{id_}", True, json.dumps(dict(rc=rc, msg=msg, tag_kept=_ops().last_attention_kernel() == before,
                                                 out_kept=bool((out == -3.0).all()))))


def case_refusals():
    B, T, H = 4, 8, 2
    q, k, v, gate, table = A.family_inputs("model", B, T, H, seed=7)
    op = Operands(q, k, v, gate, table)
    set_knobs(())
    _, _, before = op.launch()                                    # a launch that works: the tag the refusals must leave in place
    a = (op.qkv, op.gate, op.table)
    for i, name in enumerate(("qkv", "gate", "table")):
        _refusal(f"null-{name}", before, lambda out, i=i: raw(*[None if j == i else t for j, t in enumerate(a)], B, T, H, out))
    rc, msg = raw(*a, B, T, H, None)
    note("refuse/null-out", True, json.dumps(dict(rc=rc, msg=msg, tag_kept=_ops().last_attention_kernel() == before, out_kept=True)))
    _refusal("T0", before, lambda out: raw(*a, B, 0, H, out))
    _refusal("heads0", before, lambda out: raw(*a, B, T, 0, out))
    off = misaligned(op.qkv.cpu().numpy())
    _refusal("misaligned-qkv", before, lambda out: raw(off, op.gate, op.table, B, T, H, out))
    flat = torch.full((B * T * H * A.HD + 1,), -3.0, device=DEV)
    rc, msg = raw(*a, B, T, H, flat[1:])
    torch.cuda.synchronize()
    note("refuse/misaligned-out", True, json.dumps(dict(rc=rc, msg=msg, tag_kept=_ops().last_attention_kernel() == before,
                                                        out_kept=bool((flat == -3.0).all()))))
    if FP32:
        _refusal("fp32-kv_split", before, lambda out: raw(*a, B, T, H, out, 0, 1))
        _refusal("fp32-out_split", before, lambda out: raw(*a, B, T, H, out, 1, 0))
    else:
        _refusal("wide-kv_split", before, lambda out: raw(*a, B, T, H, out, 4, 1))
        _refusal("wide-out_split", before, lambda out: raw(*a, B, T, H, out, 4 | 1, 0))
    # one frame more than the longest T a kernel's LDS formula admits: refused before anything is launched.  The operands are
    # allocated in full (zeros: nothing would run on them, and a launch that slipped through would stay inside them)
    for tag, env in A.TOO_LONG.items():
        if not _mine(tag):
            continue
        T1 = A.longest_T(tag) + 1
        z = Operands(*(torch.zeros(s) for s in ((1, T1, 1, A.HD),) * 3 + ((1, T1, 1), (1, 2 * T1 - 1))))
        set_knobs(env)
        big = torch.full((T1, A.HD), -3.0, device=DEV)
        rc, msg = raw(z.qkv, z.gate, z.table, 1, T1, 1, big, 4 if tag == A.TAG_3 else 0)
        torch.cuda.synchronize()
        note(f"refuse/too-long-{A.SHORT[tag]}", True, json.dumps(dict(rc=rc, msg=msg, tag_kept=_ops().last_attention_kernel() == before,
                                                                      out_kept=bool((big == -3.0).all()))))
    set_knobs(())


def case_routes():
    note("route/asked", True, json.dumps(dict(launches=ROUTES[0], differing=ROUTES[1][:8])))


CASES = [("rows", case_rows), ("bucket", case_bucket), ("batch", case_batch), ("refusals", case_refusals), ("routes", case_routes)]

if __name__ == "__main__":
    if not FP32:
        os.environ.pop("KNNSVC_ATTENTION", None)                 # the f16x2 default, whatever the caller's environment says
    sys.exit(run_cases(CASES, sys.argv[1]))
