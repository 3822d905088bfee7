"""Child interpreter of tests/test_gpu_small_kernels.py: runs the small kernels between the stages (csrc/elementwise.hip,
csrc/synth.hip, and absmax / mean3 / axpy of csrc/conv_gemm.hip) at the shapes where each takes another branch, and writes a
JSON report {check name: {"ok": bool, "detail": str}}; the pytest process only reads it (it must not initialise the GPU itself).

    python tests/small_kernels_child.py REPORT.json

References and case generators are in tests/small_kernels_oracle.py (CPU only).  Each comparison uses the first rule that
applies, and says which in its detail:
  rule 1, bits     a copy, a select, or fp32 IEEE arithmetic in a fixed order with contraction off: bit equality with the same
                   sequence of fp32 operations in torch on the CPU (or with another launch of the kernel)
  rule 2, bound    the bound an existing test has for the kernel on the same input distribution (the test is named in the detail)
  rule 3, 4x       the reference is fp64; the yardstick is the error of the plain fp32 torch evaluation of the same operation on
                   the same inputs against it, and the bound is four times that: both sides are fp32 evaluations in different
                   orders, and the factor covers the order and the device's 1 to 2 ulp hypotf / expf / sinf.  The yardstick is
                   never taken below half an fp32 ulp of the result (2^-24 relative; of the largest |reference| where the error is
                   absolute): no fp32 evaluation can promise less, and a case of a few elements can measure less by luck.
                   Nothing in the bound comes from the kernel's output.
A split (f16x2) output adds the split's own 2^-22 relative error (ops.split_unpack) to either bound.
Outputs are views into buffers with 64 guard rows of SENTINEL on both sides and SENTINEL in the padding columns; every case also
notes that both are untouched."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np
import torch

import small_kernels_oracle as O
from knn_svc_amd import _lib, ops
from knn_svc_amd.ops import _p, _stream
from oracle import prematch_ref, synth_ref
from tests.gpu_child import DEV, SENTINEL, guarded, misaligned, note, run_cases, same

HALF_ULP = 2.0 ** -24
SPLIT_REL = 2.0 ** -22
WORST = {}                   # (family, rule) -> [checks, error / bound, error, bound, key]: what profiles/small_kernels_errors.txt lists


def lib_call(name, *args):
    _lib.check(getattr(_lib.load(), name)(*args, _stream()), name)


def worst(key, rule, err, bound):
    r = err / bound if bound > 0 else (0.0 if err == 0 else float("inf"))
    w = WORST.setdefault((key.split("/")[0], rule), [0, -1.0, 0.0, 0.0, ""])
    w[0] += 1
    if r > w[1]:
        w[1:] = [r, err, bound, key]


def err_abs(got, ref):
    d = (got.detach().cpu().double() - ref.double()).abs()
    return float(d.max()) if d.numel() else 0.0


def err_rel(got, ref):
    """Largest |got - ref| / |ref|; where the reference is exactly zero the result has to be zero (else inf)."""
    got, ref = got.detach().cpu().double(), ref.double()
    d = (got - ref).abs()
    nz = ref != 0
    e = float((d[nz] / ref[nz].abs()).max()) if bool(nz.any()) else 0.0
    return float("inf") if bool((d[~nz] != 0).any()) else e


def bits(key, got, want, what="the same fp32 operations in torch on the CPU"):
    ok = same(got, want)
    n = -1 if got is None or want is None or got.shape != want.shape else int((got.cpu().view(torch.int32) != want.cpu().view(torch.int32)).sum())
    note(key, ok, f"rule 1, bits: against {what}; {n} elements differ")
    worst(key, 1, float(n if n >= 0 else 1), 0.0)


def noted_bits(key, ok, detail):
    """A bit comparison of a single value (a range slot), or a yes / no about bits: noted, and counted under rule 1."""
    note(key, ok, detail)
    worst(key, 1, 0.0 if ok else 1.0, 0.0)


def bound2(key, got, ref, bound, cite, rel=False, split_of=None):
    e = (err_rel if rel else err_abs)(got, ref)
    b = bound + (SPLIT_REL * float(split_of.abs().max()) if split_of is not None else 0.0)
    note(key, e <= b, f"rule 2, bound of {cite}: {'rel' if rel else 'abs'} error {e:.3e} <= {b:.3e}")
    worst(key, 2, e, b)


def yard4(key, got, ref, plain, rel=False, split_of=None):
    """rule 3: ``plain`` is the fp32 torch evaluation, ``ref`` the fp64 reference."""
    f = err_rel if rel else err_abs
    y = f(plain, ref)
    floor = HALF_ULP * (1.0 if rel else float(ref.abs().max()) if ref.numel() else 0.0)
    b = 4.0 * max(y, floor) + (SPLIT_REL * float(split_of.abs().max()) if split_of is not None else 0.0)
    e = f(got, ref)
    note(key, e <= b, f"rule 3, 4x: {'rel' if rel else 'abs'} yardstick {y:.3e} (floor {floor:.3e}), bound {b:.3e}, error {e:.3e}")
    worst(key, 3, e, b)


def padded(rows, cols, ld):
    """A guarded [rows, ld] buffer -> (the [rows, cols] view, a function: guards and padding columns still hold the sentinel?)."""
    full, untouched = guarded(rows, ld)

    def clean():
        return untouched() and bool((full[:, cols:] == SENTINEL).all())
    return full[:, :cols], clean


def guards(key, *clean):
    note(key, all(c() for c in clean), "guard rows and padding columns still hold the sentinel")


def put(view, host):
    view.copy_(host.to(DEV))
    return view


# ------------------------------------------------------------------ layernorm
def run_layernorm(x_host, ga, be, gelu, split=False):
    """-> (the output view, clean()): x sits in a buffer of row stride dim + 8, the output in one of dim + 32."""
    rows, dim = x_host.shape
    x, xclean = padded(rows, dim, dim + 8)
    put(x, x_host)
    out, oclean = padded(rows, dim, dim + 32)
    ops.layernorm(x, ga, be, gelu=gelu, out=out, out_split=split)
    return out, lambda: xclean() and oclean()


def case_layernorm():
    cite = "test_gpu_kernels.test_layernorm_gelu"
    for dim in O.LN_DIMS:
        for rows in O.LN_ROWS:
            x, ga, be = O.layernorm_inputs(rows, dim)
            gad, bed = ga.to(DEV), be.to(DEV)
            for gelu in (False, True):
                key = f"layernorm/dim{dim}_rows{rows}_gelu{int(gelu)}_ld"
                ref = O.layernorm(x.double(), ga.double(), be.double(), gelu)
                out, clean = run_layernorm(x, gad, bed, gelu)
                bound2(f"{key}/fp64", out, ref, 1e-5, cite)
                guards(f"{key}/guards", clean)
                if dim % 32 == 0:
                    out, clean = run_layernorm(x, gad, bed, gelu, split=True)
                    note(f"{key}/split-guards", clean(), "guard rows and padding columns still hold the sentinel")
                    bound2(f"{key}/split-fp64", ops.split_unpack(out), ref, 1e-5, cite, split_of=ref)
                if rows == 17 and gelu:
                    alone = torch.cat([run_layernorm(x[r:r + 1], gad, bed, True)[0] for r in range(rows)])
                    bits(f"layernorm/dim{dim}_rows17_each-row-alone/bits", run_layernorm(x, gad, bed, True)[0], alone,
                         "each row in a launch of its own")
        x, ga, be = O.layernorm_inputs(3, dim, "constant")
        out, clean = run_layernorm(x, ga.to(DEV), be.to(DEV), False)
        bits(f"layernorm/dim{dim}_constant-rows-give-beta/bits", out, be[None].expand(3, dim).contiguous(), "beta")
        x, ga, be = O.layernorm_inputs(17, dim, "offset")
        out, clean = run_layernorm(x, ga.to(DEV), be.to(DEV), True)
        yard4(f"layernorm/dim{dim}_rows17_offset1000/fp64", out, O.layernorm(x.double(), ga.double(), be.double(), True),
              O.layernorm(x, ga, be, True))
        guards(f"layernorm/dim{dim}_rows17_offset1000/guards", clean)


# ------------------------------------------------------------------ wavlm_conv0
C0_ROUTES = [0, []]          # launches, and those whose shape was not what the route entry had answered


def run_conv0(x, w, ga, be, k, stride, split=False):
    B, L = x.shape
    C_ = ga.numel()
    T = (L - k) // stride + 1
    out, clean = guarded(B * T, C_)
    asked = ops.conv0_route(B, T)
    lib_call("knnsvc_wavlm_conv0", _p(x), B, L, _p(w), C_, k, stride, _p(ga), _p(be), _p(out), 1 if split else 0)
    C0_ROUTES[0] += 1
    if ops.last_conv0_route() != asked:
        C0_ROUTES[1].append(f"B {B} T {T}: asked {asked}, launched {ops.last_conv0_route()}")
    return out, clean


def case_wavlm_conv0():
    for c in O.conv0_cases():
        x, w, ga, be = O.conv0_inputs(**c)
        k, stride = c["k"], c["stride"]
        key = "wavlm_conv0/c{channels}_k{k}_s{stride}_T{T}_b{batches}".format(**c)
        ref = O.conv0(x.double(), w.double(), ga.double(), be.double(), k, stride)
        plain = O.conv0(x, w, ga, be, k, stride)
        dx, dw, dg, db = (t.to(DEV) for t in (x, w, ga, be))
        out, clean = run_conv0(dx, dw, dg, db, k, stride)
        yard4(f"{key}/fp64", out, ref, plain)
        guards(f"{key}/guards", clean)
        if c["channels"] >= 256:
            out, clean = run_conv0(dx, dw, dg, db, k, stride, split=True)
            yard4(f"{key}/split-fp64", ops.split_unpack(out), ref, plain, split_of=ref)
            guards(f"{key}/split-guards", clean)
    # the multi-span route: a workgroup walks three spans through both LDS buffers and breaks
    c = O.C0_MULTISPAN
    key = "wavlm_conv0/multispan_c{channels}_k{k}_s{stride}_T{T}_b{batches}".format(**c)
    x, w, ga, be = O.conv0_inputs(**c)
    k, stride, T, B = c["k"], c["stride"], c["T"], c["batches"]
    note(f"{key}/takes-the-multi-span-route", O.conv0_subs(T, B) > 1 and O.conv0_subs(T, 64) == 1,
         f"spans per workgroup by the dispatcher's rule: {O.conv0_subs(T, B)} for {B} batches, {O.conv0_subs(T, 64)} for 64")
    dx, dw, dg, db = (t.to(DEV) for t in (x, w, ga, be))
    out, clean = run_conv0(dx, dw, dg, db, k, stride)
    g = O.rng(8)
    rows = torch.cat([torch.randint(0, B * T, (300,), generator=g),
                      torch.tensor([0, 63, 64, 127, 128, 129, B * T - 130, B * T - 3, B * T - 2, B * T - 1])])
    yard4(f"{key}/sampled-rows-fp64", out[rows.to(DEV)], O.conv0(x.double(), w.double(), ga.double(), be.double(), k, stride, rows),
          O.conv0(x, w, ga, be, k, stride, rows))
    guards(f"{key}/guards", clean)
    single = torch.cat([run_conv0(dx[b:b + 64].contiguous(), dw, dg, db, k, stride)[0] for b in range(0, B, 64)])
    bits(f"{key}/equals-single-span-launches/bits", out, single, "the same batches in launches of 64 (one span per workgroup)")
    note("wavlm_conv0/route-entry-equals-every-launch", C0_ROUTES[0] > 0 and not C0_ROUTES[1],
         f"ops.conv0_route before against ops.last_conv0_route() after each of {C0_ROUTES[0]} launches; differing: {C0_ROUTES[1][:5]}")


# ------------------------------------------------------------------ wavlm_gate
def case_wavlm_gate():
    w2, b2, grep_a = O.gate_weights()
    dw2, db2, da = w2.to(DEV), b2.to(DEV), grep_a.to(DEV)
    for heads in (1, 12, 16):
        for rows in (1, 5):
            x = torch.randn(rows, heads * 64, generator=O.rng(9, heads, rows))
            for split in (False, True):
                key = f"wavlm_gate/heads{heads}_rows{rows}_ld{'_split' if split else ''}"
                xin = ops.split_pack(x) if split else x
                xref = ops.split_unpack(xin) if split else x              # what the kernel reads, exactly
                xd, xclean = padded(rows, heads * 64, heads * 64 + 32)
                put(xd, xin)
                out, oclean = guarded(rows, heads)
                lib_call("knnsvc_wavlm_gate", _p(xd), rows, heads, 64, xd.stride(0), _p(dw2), _p(db2), _p(da),
                         _p(out), 1 if split else 0)
                bound2(f"{key}/fp64", out, O.gate(xref.double(), heads, w2.double(), b2.double(), grep_a.double()), 1e-5,
                       "test_gpu_kernels.test_attention_and_gate")
                guards(f"{key}/guards", xclean, oclean)


# ------------------------------------------------------------------ mask_rows
def case_mask_rows():
    B, T, dim, ld = 4, 50, 64, 96
    lens = [0, 50, 17, 77]                        # the fourth is longer than T: nothing to clear
    x, clean = padded(B * T, dim, ld)
    host = torch.randn(B * T, dim, generator=O.rng(10))
    put(x, host)
    full = torch.full((B * T, ld), SENTINEL)
    full[:, :dim] = host
    ops.mask_rows(x, B, T, torch.tensor(lens, dtype=torch.int32, device=DEV))
    key = "mask_rows/B4_T50_dim64_ld96"
    bits(f"{key}/bits", x, O.mask_rows(full, B, T, dim, lens)[:, :dim], "zero rows from len on, every other bit kept")
    noted_bits(f"{key}/len-above-T-is-a-no-op", same(x[3 * T:], host[3 * T:].to(DEV)), "rule 1, bits: batch item 3 (len 77 > T 50) unchanged")
    guards(f"{key}/guards", clean)


# ------------------------------------------------------------------ reflect_pad, reflect_pad_batch
def case_reflect_pad():
    for n, pad in ((1, 0), (2, 1), (201, 200), (1000, 200), (257, 0)):
        x = torch.randn(n, generator=O.rng(11, n, pad))
        key = f"reflect_pad/n{n}_pad{pad}"
        buf, clean = padded(1, n + 2 * pad, n + 2 * pad + 112)        # the 112 floats behind belong to the caller
        dx = x.to(DEV)
        lib_call("knnsvc_reflect_pad", _p(dx), n, pad, _p(buf))
        bits(f"{key}/bits", buf[0], O.reflect_pad(x, pad))
        guards(f"{key}/guards", clean)
        bits(f"{key}_extra112/bits", ops.reflect_pad(dx, pad, extra=112), O.reflect_pad(x, pad, 112))


def case_reflect_pad_batch():
    lens, pad = [201, 1000, 4097, 202], 200
    offs = [0]
    for n in lens:
        offs.append(offs[-1] + n)
    x = torch.randn(offs[-1], generator=O.rng(12))
    dx, doffs = x.to(DEV), torch.tensor(offs, dtype=torch.int64, device=DEV)
    for stride in (max(lens) + 2 * pad + 3, 600000):                  # 600 000 > 2048 blocks x 256 threads: a second pass of the grid
        key = f"reflect_pad_batch/pad{pad}_stride{stride}"
        out, clean = guarded(len(lens), stride)
        lib_call("knnsvc_reflect_pad_batch", _p(dx), _p(doffs), len(lens), pad, _p(out), stride)
        bits(f"{key}/bits", out, O.reflect_pad_batch(x, offs, pad, stride), "the reflection and zero tails")
        guards(f"{key}/guards", clean)


# ------------------------------------------------------------------ complex_mag, harmonic_amps, spec_harm
def run_reim(v):
    rows, bins = v.shape[0], v.shape[1] // 2
    reim, clean = padded(rows, 2 * bins, 2 * bins + 6)
    put(reim, v)
    return reim, clean


def case_side_features():
    for bins in O.HARM_BINS:
        for rows in O.HARM_ROWS:
            v = O.reim_inputs(rows, bins)
            reim, rclean = run_reim(v)
            out, oclean = guarded(rows, bins)
            lib_call("knnsvc_complex_mag", _p(reim), rows, bins, reim.stride(0), _p(out))
            key = f"complex_mag/bins{bins}_rows{rows}_ld"
            yard4(f"{key}/fp64", out, O.complex_mag(v.double(), bins), O.complex_mag(v, bins), rel=True)
            guards(f"{key}/guards", rclean, oclean)
    for i, (bins, n_harm, f0) in enumerate(O.harmonic_cases()):
        rows = len(f0)
        v = O.reim_inputs(rows, bins)
        f0t = torch.from_numpy(f0)
        df0 = f0t.to(DEV)
        tag = f"bins{bins}_rows{rows}_h{n_harm}_f{i % 3}"
        # harmonic_amps on a spectrum made on the CPU: the specification is the oracle with the fp32 bin choice
        spec = O.complex_mag(v, bins)
        harm, hclean = guarded(rows, n_harm)
        dspec = spec.to(DEV)
        lib_call("knnsvc_harmonic_amps", _p(dspec), _p(df0), rows, bins, n_harm, _p(harm))
        yard4(f"harmonic_amps/{tag}/fp64", harm, O.harmonic_amps64(spec, f0t, n_harm), synth_ref.harmonic_amps(spec, f0t, n_harm), rel=True)
        guards(f"harmonic_amps/{tag}/guards", hclean)
        # spec_harm == complex_mag, then harmonic_amps on its output
        reim, rclean = run_reim(v)
        mag = ops.complex_mag(reim, bins)
        two = ops.harmonic_amps(mag, df0, n_harm)
        s1, sclean = guarded(rows, bins)
        h1, h1clean = guarded(rows, n_harm)
        lib_call("knnsvc_spec_harm", _p(reim), rows, bins, reim.stride(0), _p(df0), n_harm, _p(s1), _p(h1))
        bits(f"spec_harm/{tag}/spec-bits", s1, mag, "knnsvc_complex_mag")
        bits(f"spec_harm/{tag}/harm-bits", h1, two, "knnsvc_harmonic_amps on knnsvc_complex_mag's output")
        guards(f"spec_harm/{tag}/guards", rclean, sclean, h1clean)


# ------------------------------------------------------------------ additive_synth
def run_synth(f0, amp, pw, pb, hop, mode, want_exc, n_dyn=None, frames=None):
    """-> (cond view [N * hop, n_ch] in a buffer of n_ch + 32 columns, exc or None, clean()); ``frames``: launch only the first."""
    N = f0.numel() if frames is None else frames
    n_ch = pb.numel()
    cond, cclean = padded(N * hop, n_ch, n_ch + 32)
    exc, eclean = guarded(N * hop) if want_exc else (None, lambda: True)
    ph = torch.empty(N, device=DEV, dtype=torch.float64)
    lib_call("knnsvc_additive_synth", _p(f0), _p(amp), N, amp.shape[1] if amp is not None else 0, hop, 16000, mode, _p(pw), _p(pb), n_ch,
             _p(cond), cond.stride(0), _p(exc), _p(ph), _p(n_dyn))
    return cond, exc, lambda: cclean() and eclean()


def case_additive_synth():
    cite = "test_gpu_kernels.test_additive_synth"
    for mode, N, hop, H, n_ch, want_exc, zero_f0 in O.synth_cases():
        f0, amp, pw, pb = O.synth_inputs(N, max(H, 1), n_ch, zero_f0)
        key = f"additive_synth/mode{mode}_N{N}_hop{hop}_H{H}_ch{n_ch}{'_f0zero' if zero_f0 else ''}"
        cond, exc, clean = run_synth(f0.to(DEV), amp.to(DEV) if mode == 0 else None, pw.to(DEV), pb.to(DEV), hop, mode, want_exc)
        if mode == 0:
            ref = synth_ref.additive_synth(f0[None, :, None], amp[None], hop=hop)[0, :, 0]
            bound2(f"{key}/cond", cond, O.prenet(ref, pw, pb), 5e-5, cite)
            if want_exc:
                bound2(f"{key}/exc", exc, ref, 2e-5, cite)
        else:
            ref = O.sine_excitation64(f0, hop=hop)
            plain = synth_ref.sine_excitation(f0[None, :, None], hop=hop)[0, 0]
            yard4(f"{key}/cond", cond, O.prenet(ref, pw.double(), pb.double()), O.prenet(plain, pw, pb))
            if want_exc:
                yard4(f"{key}/exc", exc, ref, plain)
        guards(f"{key}/guards", clean)
    # a launch sized for a bucket with the valid frame count on the device: f0 and amp are NaN past the count
    hop, H, n_ch = 320, 49, 32
    launches = [(N, nd, 0) for N in O.SYNTH_DYN_N for nd in O.synth_dyn_counts(N)] + [O.SYNTH_DYN_CROSSING + (m,) for m in (0, 1)]
    for N, nd, mode in launches:
        f0, amp, pw, pb = O.synth_inputs(N, H, n_ch)
        key = f"additive_synth/dyn_N{N}_n{nd}" + ("_mode1" if mode else "")
        v = min(nd, N)
        f0[v:] = float("nan"); amp[v:] = float("nan")
        df0, damp, dpw, dpb = f0.to(DEV), amp.to(DEV) if mode == 0 else None, pw.to(DEV), pb.to(DEV)
        cond, exc, clean = run_synth(df0, damp, dpw, dpb, hop, mode, True, n_dyn=torch.tensor([nd], dtype=torch.int32, device=DEV))
        clean2 = lambda: True
        if v:
            c2, e2, clean2 = run_synth(df0, damp, dpw, dpb, hop, mode, True, frames=v)
            bits(f"{key}/valid-frames-equal-the-exact-launch/bits", torch.cat([cond[:v * hop].reshape(-1), exc[:v * hop]]),
                 torch.cat([c2.reshape(-1), e2]), f"cond and exc of a launch of exactly {v} frames")
        else:
            noted_bits(f"{key}/valid-frames-equal-the-exact-launch/bits", True, "rule 1, bits: no valid frame")
        zero = bool((cond[v * hop:] == 0).all()) and bool((exc[v * hop:] == 0).all())
        noted_bits(f"{key}/frames-past-the-count-are-zero", zero, f"rule 1, bits: cond rows and exc of frames {v}..{N - 1} are zero")
        guards(f"{key}/guards", clean, clean2)


# ------------------------------------------------------------------ absmax
def slot_value(slot):
    """What a consumer reads: the largest of the 64 stripes by the bits of |x| (kn_slot_max, include/knnsvc_hip.h)."""
    return O.abs_bits_max(slot.view(64, 32)[:, 0])


def eq_bits(a, b):
    return np.float32(a).view(np.uint32) == np.float32(b).view(np.uint32)


def case_absmax():
    host = torch.randn(5, 37, generator=O.rng(13))
    host[4, 36] = -9.5                                   # the maximum in the last column: the column tail (37 % 4 = 1)
    x, clean = padded(5, 37, 40)                         # the padding's sentinel is far larger than any element
    put(x, host)
    s = ops.absmax(x)
    noted_bits("absmax/5x37_ld40/bits", eq_bits(slot_value(s), 9.5), f"rule 1, bits: slot {slot_value(s)} against 9.5 (float4 path with a column tail)")
    guards("absmax/5x37_ld40/guards", clean)
    s = ops.absmax(misaligned(host.numpy()))
    noted_bits("absmax/5x37_misaligned/bits", eq_bits(slot_value(s), 9.5), f"rule 1, bits: slot {slot_value(s)} against 9.5 (scalar path: pointer off 16 bytes)")
    s = ops.absmax(host.to(DEV))
    noted_bits("absmax/5x37_ld37/bits", eq_bits(slot_value(s), 9.5), f"rule 1, bits: slot {slot_value(s)} against 9.5 (scalar path: ld % 4 != 0)")
    one = torch.randn(1027, generator=O.rng(14))
    s = ops.absmax(one.to(DEV))
    noted_bits("absmax/1d_1027/bits", eq_bits(slot_value(s), O.abs_bits_max(one)), f"rule 1, bits: slot {slot_value(s)} against {O.abs_bits_max(one)}")
    neg = -torch.rand(5, 37, generator=O.rng(15)) - 0.5
    s = ops.absmax(put(padded(5, 37, 40)[0], neg))
    noted_bits("absmax/all-negative/bits", eq_bits(slot_value(s), O.abs_bits_max(neg)), f"rule 1, bits: slot {slot_value(s)} against {O.abs_bits_max(neg)}")
    for name, pos in (("first", (0, 0)), ("tail-column", (2, 36)), ("last", (4, 36))):
        bad = host.clone()
        bad[pos] = float("nan")
        s = ops.absmax(put(padded(5, 37, 40)[0], bad))
        noted_bits(f"absmax/nan-{name}/bits", bool(np.isnan(slot_value(s))), f"rule 1, bits: slot {slot_value(s)} has to be NaN")
    s = ops.new_slot(DEV)
    s[0] = 1.0e6
    ops.absmax(host.to(DEV), s)
    noted_bits("absmax/keeps-a-larger-slot/bits", eq_bits(slot_value(s), 1.0e6), f"rule 1, bits: slot {slot_value(s)} against the 1e6 it held")
    s = ops.new_slot(DEV)
    s[32] = 0.25
    dhost = host.to(DEV)
    lib_call("knnsvc_absmax", _p(dhost), 0, 37, 37, _p(s))
    want = torch.zeros(ops.SLOT_W)
    want[32] = 0.25
    bits("absmax/rows0-leaves-the-slot/bits", s, want, "the slot as it was")
    big = torch.randn(64, 516, generator=O.rng(16))                       # five blocks: five stripes
    big[40, 300] = 77.0
    s = ops.absmax(big.to(DEV))
    stripes = s.view(64, 32).cpu()
    ok = eq_bits(slot_value(s), 77.0) and int((stripes[:, 0] != 0).sum()) > 1 and bool((stripes[:, 1:] == 0).all())
    noted_bits("absmax/slot-is-the-maximum-over-its-stripes/bits", ok,
         f"rule 1, bits: {int((stripes[:, 0] != 0).sum())} stripes written, their maximum {slot_value(s)} against 77, the floats between them zero")


# ------------------------------------------------------------------ mean3, axpy
def case_mean3_axpy():
    for n in O.MEAN3_N:
        g = O.rng(17, n)
        a, b, c = (torch.randn(n, generator=g) for _ in range(3))
        da, db, dc = a.to(DEV), b.to(DEV), c.to(DEV)
        for div in (1.0, 3.0, 7.0):
            key = f"mean3/n{n}_div{int(div)}"
            out, clean = guarded(n)
            slot = ops.new_slot(DEV)
            ops.mean3(da, db, dc, div, out, slot)
            want = O.mean3_f32(a, b, c, div)
            bits(f"{key}/bits", out, want)
            noted_bits(f"{key}/slot-bits", eq_bits(slot_value(slot), O.abs_bits_max(want)), f"rule 1, bits: slot {slot_value(slot)} against max |out| {O.abs_bits_max(want)}")
            guards(f"{key}/guards", clean)
        for acc in (0, 1):
            key = f"axpy/n{n}_acc{acc}"
            out, clean = guarded(n)
            put(out, c)
            ops.axpy(da, 0.37, out, acc)
            bits(f"{key}/bits", out, O.axpy_f32(a, 0.37, c, acc))
            guards(f"{key}/guards", clean)
    # the device-side count: only count * (n / bucket frames) floats are read and written
    n, frames = 1028, 257
    g = O.rng(18)
    a, b, c = (torch.randn(n, generator=g) for _ in range(3))
    for count in (0, 128, 300):
        cut = min(count, frames) * (n // frames)
        ap = a.clone()
        ap[cut:] = 1.0e9                                   # what lies past the cut must not reach the slot
        key = f"mean3/dyn_n{n}_count{count}"
        out, clean = guarded(n)
        slot = ops.new_slot(DEV)
        ops.mean3(ap.to(DEV), b.to(DEV), c.to(DEV), 3.0, out, slot, dyn=(torch.tensor([count], dtype=torch.int32, device=DEV), frames))
        want = torch.full((n,), SENTINEL)
        want[:cut] = O.mean3_f32(ap, b, c, 3.0)[:cut]
        bits(f"{key}/bits", out, want, "the mean before the cut, the sentinel behind it")
        noted_bits(f"{key}/slot-bits", eq_bits(slot_value(slot), O.abs_bits_max(want[:cut])), f"rule 1, bits: slot {slot_value(slot)} against {O.abs_bits_max(want[:cut])}")
        guards(f"{key}/guards", clean)


# ------------------------------------------------------------------ weighted_gather, amp_ratio, round_f16
def case_match_helpers():
    for k in O.GATHER_K:
        for dim in O.GATHER_DIM:
            idx, w, pool = O.gather_inputs(k, dim)
            key = f"weighted_gather/k{k}_dim{dim}_ld"
            dpool, pclean = padded(pool.shape[0], dim, dim + 5)
            put(dpool, pool)
            didx = idx.to(DEV)
            outs = {}
            for name, dw, mode in (("given", w.to(DEV), 0), ("uniform0", None, 0), ("uniform1", None, 1)):
                out, oclean = guarded(idx.shape[0], dim)
                lib_call("knnsvc_weighted_gather", _p(didx), _p(dw), idx.shape[0], k, _p(dpool), dim, dpool.stride(0), mode, _p(out))
                outs[name] = out
                guards(f"{key}/{name}-guards", pclean, oclean)
            bound2(f"{key}/given-fp64", outs["given"], O.weighted_gather(idx, w.double(), pool.double()), 1e-5, "test_gpu_kernels.test_smooth_weights")
            bits(f"{key}/uniform0-bits", outs["uniform0"], O.uniform_gather_f32(idx, pool, 0))
            bits(f"{key}/uniform1-bits", outs["uniform1"], O.uniform_gather_f32(idx, pool, 1))
            if k & (k - 1) == 0:
                bits(f"{key}/modes-agree-bits", outs["uniform0"], outs["uniform1"], "the other mean mode (k is a power of two)")
    for nq in O.AMP_NQ:
        for k in O.AMP_K:
            for bins in O.AMP_BINS:
                sq, sp, idx = O.amp_ratio_inputs(nq, k, bins)
                key = f"amp_ratio/nq{nq}_k{k}_bins{bins}_ld"
                dq, qclean = padded(nq, bins, bins + 3)
                dp, pclean = padded(sp.shape[0], bins, bins + 5)
                put(dq, sq); put(dp, sp)
                out, oclean = guarded(nq, k)
                didx = idx.to(DEV)
                lib_call("knnsvc_amp_ratio", _p(dq), dq.stride(0), _p(dp), dp.stride(0), sp.shape[0], _p(didx), nq, k, bins, _p(out))
                bound2(f"{key}/fp64", out, prematch_ref.amp_ratio(sq.double(), sp.double(), idx), 2e-6,
                       "test_gpu_kernels.test_round_f16_and_amp_ratio", rel=True)
                guards(f"{key}/guards", qclean, pclean, oclean)
    for n in O.ROUND_N:
        x = O.round_f16_inputs(n)
        out, clean = guarded(n)
        dx = x.to(DEV)
        lib_call("knnsvc_round_f16", _p(dx), n, _p(out))
        bits(f"round_f16/n{n}/bits", out, O.round_f16(x), "x.half().float()")
        guards(f"round_f16/n{n}/guards", clean)


def case_summary():
    """One entry per family and rule: the largest error against its bound and where (rule 1: the elements that differ)."""
    for fam, rule in sorted(WORST):
        n, r, e, b, key = WORST[(fam, rule)]
        note(f"summary/{fam}/rule{rule}", True, f"{n} bit comparisons, " + ("all equal" if e == 0 else f"{key} differs") if rule == 1 else
             f"{n} comparisons, largest error {e:.3e} against its bound {b:.3e} (ratio {r:.2f}) at {key}")


if __name__ == "__main__":
    sys.exit(run_cases([("layernorm_cases", case_layernorm), ("wavlm_conv0_cases", case_wavlm_conv0), ("wavlm_gate_cases", case_wavlm_gate),
                        ("mask_rows_cases", case_mask_rows), ("reflect_pad_cases", case_reflect_pad),
                        ("reflect_pad_batch_cases", case_reflect_pad_batch), ("side_feature_cases", case_side_features),
                        ("additive_synth_cases", case_additive_synth), ("absmax_cases", case_absmax),
                        ("mean3_axpy_cases", case_mean3_axpy), ("match_helper_cases", case_match_helpers),
                        ("summary", case_summary)], sys.argv[1]))
