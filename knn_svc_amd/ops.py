"""Thin tensor-level wrappers over the C ABI (include/knnsvc_hip.h).

PyTorch-ROCm is used for device memory and streams only: every function takes
contiguous fp32 tensors on the GPU, passes raw device pointers plus the current
HIP stream to ``libknnsvc_hip.so`` and returns tensors.  No op has a torch
fallback — a missing library or a CPU tensor raises.
"""
from __future__ import annotations

import ctypes as C
import math
import os
import threading
from collections import namedtuple

import torch

from . import _lib
from ._lib import ConvDesc, KnnSvcError, PairDesc, check

ACT_NONE, ACT_GELU, ACT_LRELU, ACT_TANH = 0, 1, 2, 3


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def _need(t, dtype=torch.float32, name="tensor"):
    if not (isinstance(t, torch.Tensor) and t.is_cuda):
        raise KnnSvcError(f"{name}: expected a GPU tensor (knn_svc_amd has no CPU path)")
    if t.dtype != dtype:
        raise KnnSvcError(f"{name}: expected {dtype}, got {t.dtype}")
    return t


# ------------------------------------------------------------------ weight packing (host side, once per load)
def pack_conv_weight(w: torch.Tensor) -> torch.Tensor:
    """Conv1d weight [Cout, Cin, k] -> GEMM B operand [Cout, k*Cin] (tap major, channel minor)."""
    return w.permute(0, 2, 1).reshape(w.shape[0], -1).contiguous()


def pack_grouped_conv_weight(w: torch.Tensor, groups: int) -> torch.Tensor:
    """Grouped Conv1d weight [Cout, Cin/g, k] -> [g, Cout/g, k*Cin/g]."""
    co, cig, k = w.shape
    return w.reshape(groups, co // groups, cig, k).permute(0, 1, 3, 2).reshape(groups, co // groups, k * cig).contiguous()


def pack_convT_weight(w: torch.Tensor, u: int) -> torch.Tensor:
    """ConvTranspose1d weight [Cin, Cout, k] (stride u, k % u == 0) -> [u*Cout, (k/u)*Cin] with
    row p*Cout+co, column r*Cin+c holding w[c, co, p + r*u]: output phase p of input step q sums
    x[q-r] . w[:, co, p + r*u] over the k/u taps r."""
    cin, cout, k = w.shape
    assert k % u == 0, "transposed conv kernel must be a multiple of its stride"
    r = k // u
    return w.reshape(cin, cout, r, u).permute(3, 1, 2, 0).reshape(u * cout, r * cin).contiguous()


def gemm_mode() -> str:
    """KNNSVC_GEMM = f16x2 (default) | bf16x3 | fp32: how conv_gemm evaluates fp32 products for weights that
    went through attach_split (all three keep fp32-GEMM accuracy; see gemm2_core.h / gemm3_core.h)."""
    mode = os.environ.get("KNNSVC_GEMM", "f16x2")
    if mode not in ("f16x2", "bf16x3", "fp32"):
        raise KnnSvcError(f"KNNSVC_GEMM={mode!r}: expected f16x2, bf16x3 or fp32")
    return mode


def attach_split(w: torch.Tensor) -> torch.Tensor:
    """Pre-split a packed weight matrix [..., K] (K % 32 == 0) for the emulated-fp32 matrix-core kernels and
    hang the result on the tensor: ``w._w2`` (+ ``w._w2_scale``) = two fp16 planes of scale*w with the
    per-tensor power-of-two scale that puts max|w| in [2^13, 2^14) (default), or ``w._w3`` = three bf16
    planes (KNNSVC_GEMM=bf16x3).  No-op when the shape does not qualify or KNNSVC_GEMM=fp32 is set."""
    mode = gemm_mode()
    if mode == "fp32" or not w.is_cuda or w.dtype != torch.float32:
        return w
    K = w.shape[-1]
    if K % 32 != 0 or not w.is_contiguous():
        return w
    rows = w.numel() // K
    if mode == "bf16x3":
        out = torch.empty(rows * (K // 32) * 96, device=w.device, dtype=torch.int16)
        check(_lib.load().knnsvc_split_weight_bf16x3(_p(w), rows, K, _p(out), _stream()), "split_weight")
        w._w3 = out
        return w
    wmax = float(w.abs().max())
    if not math.isfinite(wmax):
        raise KnnSvcError("attach_split: non-finite weight")
    scale = 2.0 ** (13 - math.frexp(wmax)[1] + 1) if wmax > 0 else 1.0       # max|w| * scale in [2^13, 2^14)
    scale = min(max(scale, 2.0 ** -60), 2.0 ** 60)
    out = torch.empty(rows * (K // 32) * 64, device=w.device, dtype=torch.int16)
    check(_lib.load().knnsvc_split_weight_f16x2(_p(w), rows, K, scale, _p(out), _stream()), "split_weight")
    w._w2, w._w2_scale = out, scale
    return w


_GRAPH_READY = set()


def prepare_graph_capture(device) -> None:
    """torch registers per-generator graph-state tensors at the first ``capture_begin`` on a device.  If that first
    capture happens under ``torch.inference_mode()`` (KNeighborsVC's methods are decorated with it) they become
    inference tensors, and every later capture outside inference mode dies with "Inplace update to inference tensor".
    Doing one trivial capture in normal mode first makes the capture sites order-independent."""
    idx = torch.device(device).index
    idx = torch.cuda.current_device() if idx is None else idx
    if idx in _GRAPH_READY:
        return
    with torch.inference_mode(False):
        t = torch.zeros(1, device=torch.device("cuda", idx))
        torch.cuda.synchronize(idx)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            t.add_(1.0)
        del g
    _GRAPH_READY.add(idx)


_CAPTURE_STREAMS = {}


def capture_graph(fn, device, pool=None):
    """Capture ``fn()`` (which may only enqueue kernels on the current stream and allocate torch tensors) into a hipGraph
    WITHOUT synchronising the device: ``torch.cuda.graph`` calls ``torch.cuda.synchronize()`` on entry, which would stall a
    stream pipeline that happens to meet a new shape.  Capture runs on a private side stream ordered behind the caller's
    stream.  -> (graph, fn's return value: the graph's static outputs)."""
    prepare_graph_capture(device)
    idx = torch.device(device).index
    idx = torch.cuda.current_device() if idx is None else idx
    side = _CAPTURE_STREAMS.get(idx)
    if side is None:
        from .pipeline import new_stream
        side = _CAPTURE_STREAMS[idx] = new_stream(idx, kind="capture")
    cur = torch.cuda.current_stream(idx)
    side.wait_stream(cur)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        if pool is not None:
            g.capture_begin(pool=pool, capture_error_mode="thread_local")
        else:
            g.capture_begin(capture_error_mode="thread_local")
        try:
            out = fn()
        finally:
            g.capture_end()
    cur.wait_stream(side)
    return g, out


# ------------------------------------------------------------------ implicit-GEMM convolution
def last_conv_kernel() -> str:
    """Tag of the kernel the last conv_gemm of this thread dispatched to (measurement hook)."""
    return _lib.load().knnsvc_conv_gemm_last_kernel().decode()


def last_conv_epilogue() -> str:
    """"patch" / "lane" / "": the epilogue the last conv_gemm launch of this thread took (test hook)."""
    return _lib.load().knnsvc_conv_gemm_last_epilogue().decode()


def conv_route(descs) -> tuple:
    """(tag, epilogue) the dispatcher decides for 1..4 descriptors collected with ``conv_gemm(..., defer=descs)``, asked without
    a launch (knnsvc_conv_gemm_route: host code, CPU tensors' pointers will do).  One descriptor: what last_conv_kernel() /
    last_conv_epilogue() say after its launch; several: the tag of their one grid, or "" where conv_gemm_multi launches one each."""
    arr = (ConvDesc * len(descs))(*descs)
    tag, epi = C.create_string_buffer(32), C.create_string_buffer(32)
    check(_lib.load().knnsvc_conv_gemm_route(arr, len(descs), tag, epi, 32), "conv_gemm_route")
    return tag.value.decode(), epi.value.decode()


def conv_tags() -> set:
    """Every tag last_conv_kernel() can report."""
    buf = C.create_string_buffer(512)
    check(_lib.load().knnsvc_conv_gemm_tags(buf, 512), "conv_gemm_tags")
    return set(buf.value.decode().split())


def conv_gemm(x, w, out, *, m, n, cin, taps=1, stride=1, dil=1, pad=0, t_in=None, ldx=None, ldo=None,
              bias=None, bias_period=0, act=ACT_NONE, act_slope=0.0, a_slope=1.0, resid=None, ldr=None,
              accumulate=False, div=1.0, batches=1, groups=1, x_bstride=0, x_gstride=0, w_gstride=0,
              bias_gstride=0, o_bstride=0, o_gstride=0, r_bstride=0, r_gstride=0,
              convt_u=0, convt_cout=0, convt_pad=0, t_out=0, a_scale=0.0, x_split=False, out_split=False,
              w2=None, w2_scale=0.0, x_absmax=None, w_absmax=None, out_absmax=None, out_split_scale=0.0, dyn=None, x_bound=None,
              fixed_tile=False, defer=None):
    """See knnsvc_conv_gemm.  x/out/resid may be views into wider buffers (pass ldx/ldo/ldr).
    ``x_absmax`` / ``w_absmax`` / ``out_absmax``: one-element device tensors (range slots of the f16x2 path, see the
    header): bound of |x| / |w| the kernel derives its operand scales from, and where this launch folds max|out|.
    ``defer``: a list — the descriptor is appended to it instead of being launched (``conv_gemm_multi`` launches the list)."""
    lib = _lib.load()
    d = ConvDesc()
    d.x = x.data_ptr(); d.x_bstride = x_bstride; d.x_gstride = x_gstride
    d.ldx = ldx if ldx is not None else cin; d.t_in = t_in if t_in is not None else m
    d.cin = cin; d.taps = taps; d.stride = stride; d.dil = dil; d.pad = pad; d.a_slope = a_slope
    d.w = w.data_ptr(); d.w_gstride = w_gstride; d.n = n
    d.bias = bias.data_ptr() if bias is not None else None
    d.bias_gstride = bias_gstride; d.bias_period = bias_period
    d.out = out.data_ptr(); d.o_bstride = o_bstride; d.o_gstride = o_gstride
    d.ldo = ldo if ldo is not None else n; d.m = m
    d.act = act; d.act_slope = act_slope
    d.resid = resid.data_ptr() if resid is not None else None
    d.r_bstride = r_bstride; d.r_gstride = r_gstride; d.ldr = ldr if ldr is not None else (d.ldo if resid is not None else 0)
    d.accumulate = 1 if accumulate else 0; d.div = div
    d.batches = batches; d.groups = groups
    d.convt_u = convt_u; d.convt_cout = convt_cout; d.convt_pad = convt_pad; d.t_out = t_out
    w3 = getattr(w, "_w3", None)
    d.w_bf16x3 = w3.data_ptr() if w3 is not None else None
    if w2 is None:
        w2, w2_scale = getattr(w, "_w2", None), getattr(w, "_w2_scale", 0.0)
    d.w_f16x2 = w2.data_ptr() if w2 is not None else None
    d.w_f16x2_scale = w2_scale if w2 is not None else 0.0
    d.a_f16x2_scale = a_scale
    d.x_f16x2 = 1 if x_split else 0
    d.out_f16x2 = int(out_split) if (out_split is not True and out_split is not False) else (1 if out_split else 0)   # True / first split column
    if not x_split and (x_absmax is not None or out_absmax is not None) and not range_slots_on():
        x_absmax = out_absmax = None            # A/B aid: fixed activation scale 16 (a pre-split operand keeps its slot)
    if _SLOT_DBG and not x_split:          # timing aid: KNNSVC_SLOT_DBG=x keeps only the consumer side, =o only the producer side
        if _SLOT_DBG == "x": out_absmax = None
        if _SLOT_DBG == "o": x_absmax = None
    d.x_absmax = x_absmax.data_ptr() if x_absmax is not None else None
    d.w_absmax = w_absmax.data_ptr() if w_absmax is not None else None
    d.out_absmax = out_absmax.data_ptr() if out_absmax is not None else None
    d.out_f16x2_scale = out_split_scale
    d.fixed_tile = int(fixed_tile)          # False/0: by size, 1/True: the 128x128 kernel, 2: the 256x256 (Gemm2QuadS) kernel
    if x_bound is not None:            # (mul, add): |x| <= mul * max(x_absmax slot) + add — an input that was not measured itself
        d.x_bound_mul, d.x_bound_add = float(x_bound[0]), float(x_bound[1])
    if dyn is not None:
        # dyn = (device int32 count n, the bucket's count Nb): t_in / m / t_out of THIS call are what they are at n = Nb; each is
        # affine in the count with an offset in [0, Nb) (the generator's lengths: Nb * factor, + 1 or + taps - 1), recovered here
        n_t, nb = dyn
        d.n_dyn = n_t.data_ptr()
        d.dyn_t_in_mul, d.dyn_t_in_add = divmod(int(d.t_in), nb)
        d.dyn_m_mul, d.dyn_m_add = divmod(int(m), nb)
        d.dyn_t_out_mul = int(t_out) // nb if convt_u else 0
        if convt_u and int(t_out) % nb:
            raise KnnSvcError("conv_gemm: dynamic t_out must be a multiple of the bucket count")
    if defer is not None:
        defer.append(d)
        return out
    check(lib.knnsvc_conv_gemm(C.byref(d), _stream()), "conv_gemm")
    return out


def conv_gemm_multi(descs) -> None:
    """Launch the descriptors collected with ``conv_gemm(..., defer=descs)`` — convolutions of one output shape (the generator's
    three ResBlock branches of a step) — as ONE grid (knnsvc_conv_gemm_multi); same bits as separate launches."""
    if not descs:
        return
    for i in range(0, len(descs), 4):
        part = descs[i:i + 4]
        arr = (ConvDesc * len(part))(*part)
        check(_lib.load().knnsvc_conv_gemm_multi(arr, len(part), _stream()), "conv_gemm_multi")


def resblock_pair_multi(descs) -> None:
    """The same for ``resblock_pair(..., defer=descs)`` (knnsvc_resblock_pair_multi)."""
    if not descs:
        return
    for i in range(0, len(descs), 4):
        part = descs[i:i + 4]
        arr = (PairDesc * len(part))(*part)
        check(_lib.load().knnsvc_resblock_pair_multi(arr, len(part), _stream()), "resblock_pair_multi")


def absmax(x2d, slot=None):
    """max |x| of a [rows, cols] view (row stride allowed) folded into ``slot`` (a zeroed one-element device tensor is
    made when None): the range slot a later conv_gemm takes as x_absmax / w_absmax.  NaN in x makes the slot NaN."""
    _need(x2d, name="absmax.x")
    if not range_slots_on() and slot is not None:
        return slot
    if slot is None:
        slot = new_slot(x2d.device)
    if x2d.dim() == 1:
        x2d = x2d[None]
    if x2d.stride(1) != 1:
        raise KnnSvcError("absmax: rows must be contiguous")
    check(_lib.load().knnsvc_absmax(_p(x2d), x2d.shape[0], x2d.shape[1], x2d.stride(0) if x2d.shape[0] > 1 else x2d.shape[1],
                                    _p(slot), _stream()), "absmax")
    return slot


def resblock_pair_ok(channels: int, taps: int, dil: int) -> bool:
    """The fused ResBlock pair covers the generator's narrow stages (knnsvc_resblock_pair); KNNSVC_FUSED_PAIR=0 switches it off."""
    widths = (32, 64, 128) if os.environ.get("KNNSVC_FUSED_PAIR_128", "0") == "1" else (32, 64)
    return (os.environ.get("KNNSVC_FUSED_PAIR", "1") != "0" and gemm_mode() == "f16x2" and channels in widths and
            taps % 2 == 1 and taps <= 11 and dil * (taps - 1) <= 64)


def resblock_pair(x, w1, b1, w2, b2, out, *, t, channels, taps, dil, slope, x_absmax, t1_bound, out_absmax=None, dyn=None,
                  ldx=None, ldo=None, defer=None):
    """out = conv1d(lrelu(conv1d(lrelu(x), w1, dilation=dil) + b1), w2) + b2 + x in one launch (see the header); w1 / w2 are packed
    conv weights carrying their f16x2 split (attach_split).  Bit-identical to the two conv_gemm launches."""
    d = PairDesc()
    d.x = x.data_ptr(); d.ldx = ldx if ldx is not None else channels; d.t = t; d.channels = channels; d.taps = taps; d.dil = dil
    d.w1_f16x2 = w1._w2.data_ptr(); d.w1_scale = w1._w2_scale; d.b1 = b1.data_ptr() if b1 is not None else None
    d.w2_f16x2 = w2._w2.data_ptr(); d.w2_scale = w2._w2_scale; d.b2 = b2.data_ptr() if b2 is not None else None
    d.out = out.data_ptr(); d.ldo = ldo if ldo is not None else channels
    d.slope = slope
    if range_slots_on() and x_absmax is not None:
        d.x_absmax = x_absmax.data_ptr(); d.t1_bound_mul, d.t1_bound_add = float(t1_bound[0]), float(t1_bound[1])
        d.out_absmax = out_absmax.data_ptr() if out_absmax is not None else None
    else:                                   # A/B aid (KNNSVC_RANGE_SLOTS=0): the fixed activation scale 16
        d.x_absmax = None; d.a1_scale = d.a2_scale = 16.0; d.out_absmax = None
    if dyn is not None:
        d.n_dyn = dyn[0].data_ptr(); d.dyn_mul = t // dyn[1]
    if defer is not None:
        defer.append(d)
        return out
    check(_lib.load().knnsvc_resblock_pair(C.byref(d), _stream()), "resblock_pair")
    return out


def axpy(x, alpha, out, accumulate):
    """out = alpha * x (+ out): one term of a general WavLM layer weighting."""
    check(_lib.load().knnsvc_axpy(_p(x), x.numel(), float(alpha), 1 if accumulate else 0, _p(out), _stream()), "axpy")
    return out


def mean3(a, b, c, div, out, out_absmax=None, dyn=None, row_floats=0):
    """out = (c + (b + a)) / div over contiguous tensors; ``dyn`` = (device frame count, bucket frames): only the first
    count * (numel / bucket frames) floats are touched."""
    n = a.numel()
    nd, mul = (None, 0)
    if dyn is not None:
        nd, mul = dyn[0], n // dyn[1]
    if not range_slots_on():
        out_absmax = None
    check(_lib.load().knnsvc_mean3(_p(a), _p(b), _p(c), n, float(div), _p(out), _p(out_absmax), _p(nd), mul, _stream()), "mean3")
    return out


SLOT_W = 64 * 32     # a range slot is 64 stripes of one 128-byte cache line each (float 32 i = stripe i): include/knnsvc_hip.h


def new_slot(device) -> torch.Tensor:
    return torch.zeros(SLOT_W, device=device, dtype=torch.float32)


def pick_scale(bound: float) -> float:
    """Host mirror of the kernels' kn_pick_scale: the largest power of two s with bound * s < 2^15."""
    if not (bound > 0.0) or not math.isfinite(bound):
        return 2.0 ** 54 if bound == 0.0 else 2.0 ** -114
    return 2.0 ** (14 - max(math.frexp(bound)[1] - 1, -40))


def linear(x2d, w, bias=None, act=ACT_NONE, resid=None, out=None, x_split=False, out_split=False, **kw):
    """out[M,N] = act(x2d[M,K] @ w[N,K]^T + bias) (+ resid).  x_split / out_split: operand / result in the f16x2
    split layout (include/knnsvc_hip.h, "A2"), carried in float32 tensors of the usual shape; out_split may also be
    the first split column (a multiple of 32): columns before it stay fp32."""
    _need(x2d, name="linear.x"); _need(w, name="linear.w")
    M, K = x2d.shape
    N = w.shape[0]
    if out is None:
        out = torch.empty(M, N, device=x2d.device, dtype=torch.float32)
    return conv_gemm(x2d, w, out, m=M, n=N, cin=K, bias=bias, act=act, resid=resid, x_split=x_split, out_split=out_split, **kw)


def split_pack(x2d: torch.Tensor) -> torch.Tensor:
    """fp32 [rows, C] (C % 32 == 0) -> the f16x2 split layout in a float32 tensor of the same shape (torch ops;
    for tests and debugging — the kernels write this layout themselves)."""
    rows, C = x2d.shape
    xs = x2d.float() * 16.0
    hi = xs.half()
    lo = (xs - hi.float()).half()
    packed = torch.stack([hi.view(rows, C // 32, 32), lo.view(rows, C // 32, 32)], 2).contiguous()   # [rows, C/32, 2, 32]
    return packed.view(torch.float32).view(rows, C)


def split_unpack(t2d: torch.Tensor) -> torch.Tensor:
    """inverse of split_pack (up to the 2^-22 relative split error)."""
    rows, C = t2d.shape
    h = t2d.contiguous().view(torch.float16).view(rows, C // 32, 2, 32)
    return ((h[:, :, 0].float() + h[:, :, 1].float()) / 16.0).reshape(rows, C)


# ------------------------------------------------------------------ WavLM pieces
def layernorm(x2d, gamma, beta, gelu=False, out=None, out_split=False):
    """out_split: write the f16x2 split layout (the result then only makes sense as a GEMM's x_split operand)."""
    _need(x2d, name="layernorm.x")
    rows, dim = x2d.shape
    if out is None:
        out = torch.empty_like(x2d)
    check(_lib.load().knnsvc_layernorm(_p(x2d), rows, dim, x2d.stride(0), _p(gamma), _p(beta), (1 if gelu else 0) | (2 if out_split else 0),
                                       _p(out), out.stride(0), _stream()), "layernorm")
    return out


def wavlm_conv0(x, w, gamma, beta, k, stride, out_split=False):
    """[B, L] waveform -> [B*T, C] = GELU(LN(conv1d(x))) of the first feature-extractor layer, one kernel."""
    B, L = x.shape
    C_ = gamma.numel()
    T = (L - k) // stride + 1
    out = torch.empty(B * T, C_, device=x.device, dtype=torch.float32)
    check(_lib.load().knnsvc_wavlm_conv0(_p(x), B, L, _p(w), C_, k, stride, _p(gamma), _p(beta), _p(out),
                                         1 if out_split else 0, _stream()), "wavlm_conv0")
    return out


def conv0_route(batches, T) -> tuple:
    """(rows per pass, spans of 64 rows per workgroup) wavlm_conv0 launches with for ``batches`` inputs of T frames, asked
    without a launch (knnsvc_wavlm_conv0_route)."""
    rp, spans = C.c_int32(), C.c_int32()
    check(_lib.load().knnsvc_wavlm_conv0_route(batches, T, C.byref(rp), C.byref(spans)), "wavlm_conv0_route")
    return rp.value, spans.value


def last_conv0_route() -> tuple:
    """... and what the last wavlm_conv0 of this thread launched with ((0, 0) before the first): test hook."""
    rp, spans = C.c_int32(), C.c_int32()
    _lib.load().knnsvc_wavlm_conv0_last_route(C.byref(rp), C.byref(spans))
    return rp.value, spans.value


def wavlm_gate(xn2d, heads, w2, b2, grep_a, x_split=False):
    rows = xn2d.shape[0]
    gate = torch.empty(rows, heads, device=xn2d.device, dtype=torch.float32)
    check(_lib.load().knnsvc_wavlm_gate(_p(xn2d), rows, heads, 64, xn2d.stride(0), _p(w2), _p(b2), _p(grep_a),
                                        _p(gate), 1 if x_split else 0, _stream()), "wavlm_gate")
    return gate


def attention_mode() -> str:
    """KNNSVC_ATTENTION = f16x2 (default) | bf16x3 | fp32, as knnsvc_wavlm_attention reads it."""
    e = os.environ.get("KNNSVC_ATTENTION", "")
    return "bf16x3" if e[:1] == "b" else "fp32" if e[:2] == "fp" else "f16x2"


def mask_rows(x2d, batches, T, lens):
    """Rows t >= lens[b] of the [batches*T, dim] activation become zero in place (``lens``: int32 device tensor)."""
    _need(x2d, name="mask_rows.x"); _need(lens, torch.int32, "mask_rows.lens")
    check(_lib.load().knnsvc_mask_rows(_p(x2d), batches, T, x2d.shape[1], x2d.stride(0), _p(lens), _stream()), "mask_rows")
    return x2d


def wavlm_attention(qkv, gate, table, batches, T, heads, out_split=False, kv_split=False, wide=False, kv_len=None):
    """kv_split: the K and V column blocks of qkv hold the f16x2 split layout (QKV projection run with out_split=E).
    wide: Q / K / V may exceed the f16x2 kernel's fixed-scale range (decided at load from the weights,
    WavLMEncoder._range_plan): run the bf16x3 kernel (fp32 exponent range) whatever KNNSVC_ATTENTION says."""
    if wide and (out_split or kv_split):
        raise KnnSvcError("wavlm_attention: wide-range mode has fp32 inputs and outputs")
    out = torch.empty(batches * T, heads * 64, device=qkv.device, dtype=torch.float32)
    check(_lib.load().knnsvc_wavlm_attention(_p(qkv), _p(gate), _p(table), batches, T, heads, _p(out),
                                             (1 if out_split else 0) | (4 if wide else 0), 1 if kv_split else 0, _p(kv_len),
                                             _stream()), "wavlm_attention")
    return out


def attention_route(batches, T, heads, out_split=False, kv_split=False, wide=False) -> tuple:
    """(tag, bytes of dynamic LDS) of the kernel wavlm_attention launches for these sizes and flags under the knobs as they are,
    asked without a launch (knnsvc_wavlm_attention_route); raises where wavlm_attention would refuse the call for them."""
    tag, lds = C.create_string_buffer(32), C.c_int64()
    check(_lib.load().knnsvc_wavlm_attention_route(batches, T, heads, (1 if out_split else 0) | (4 if wide else 0), 1 if kv_split else 0,
                                                   tag, 32, C.byref(lds)), "wavlm_attention_route")
    return tag.value.decode(), lds.value


def last_attention_kernel() -> str:
    """Tag of the kernel the last wavlm_attention of this thread launched ("wavlm_attention2", "wavlm_attention2q",
    "wavlm_attention2w", "wavlm_attention3", "wavlm_attention"; "" before the first launch): measurement and test hook."""
    return _lib.load().knnsvc_wavlm_attention_last_kernel().decode()


# ------------------------------------------------------------------ kNN
_SLOT_DBG = os.environ.get("KNNSVC_SLOT_DBG", "")


def range_slots_on() -> bool:
    """KNNSVC_RANGE_SLOTS=0 (A/B aid): f16x2 GEMMs fall back to the fixed activation scale 16 (|x| < 4094)."""
    return os.environ.get("KNNSVC_RANGE_SLOTS", "1") != "0"


def row_norms(x2d, slot=None):
    """-> (norm [rows], sumsq [rows]).  ``norm._slot``: one-element device tensor holding the largest row norm — an
    upper bound of max|x| the kernel folds on the way (the kNN's range slot; no extra pass over the features).
    ``slot``: a ZEROED range slot to fold into (a search zeroes all its small buffers with one fill: knn_topk)."""
    _need(x2d, name="row_norms.x")
    rows, dim = x2d.shape
    norm = torch.empty(rows, device=x2d.device, dtype=torch.float32)
    sq = torch.empty(rows, device=x2d.device, dtype=torch.float32)
    slot = new_slot(x2d.device) if slot is None else slot
    check(_lib.load().knnsvc_row_norms(_p(x2d), rows, dim, x2d.stride(0), _p(norm), _p(sq), _p(slot), _stream()), "row_norms")
    norm._slot = slot
    return norm, sq


def knn_mode() -> str:
    """KNNSVC_KNN = f16x2 | fp32.  f16x2 (default while KNNSVC_GEMM is f16x2): q.p^T from the emulated-fp32 GEMM +
    knnsvc_knn_select; fp32: the fused exact-fp32-MFMA tile kernel (knnsvc_knn_topk)."""
    mode = os.environ.get("KNNSVC_KNN", "f16x2" if gemm_mode() == "f16x2" else "fp32")
    if mode not in ("f16x2", "fp32"):
        raise KnnSvcError(f"KNNSVC_KNN={mode!r}: expected f16x2 or fp32")
    return mode


KNN_RSRC_BYTES = 1 << 30          # every buffer resource of a search stays below this: the one place the bound is written
KNN_WIDE = 64                     # keys per row of a wide list (include/knnsvc_hip.h, knnsvc_knn_rescore)
KNN_GUARD = 4.0e-6                # the wide lists keep everything within this of the k-th screening distance (csrc/knn.hip)
KNN_ROUTE_COUNTS = {"chunks": 0, "fused": 0, "dot": 0}     # which route each (search, pool chunk) took: tests assert on it
# The fused route (epochs of knnsvc_knn_screen + knnsvc_knn_refine, no dot matrix) from 256 query frames x 8192 pool rows on.
# Round 3 (threshold from a separate sample pass: ~0.15 ms whatever the size) had 2048 / 8192; round 2 4096 / 32768.
KNN_FUSED_MIN_Q = int(os.environ.get("KNNSVC_KNN_FUSED_MIN_Q", "256"))
KNN_FUSED_MIN_P = int(os.environ.get("KNNSVC_KNN_FUSED_MIN_P", "8192"))
KNN_FUSED_CAP = 4096
KNN_OVERFLOW = 2                  # flag bit: the fused route's candidate buffer overflowed
KNN_DEBUG_COUNTS = None
KNN_EPOCH_GROWTH = int(os.environ.get("KNNSVC_KNN_EPOCH_GROWTH", "4"))
KNN_COLD_TILES_MAX = 44           # column tiles of the first epoch: ~45 candidates per (row, tile) have to fit the buffer twice over
_FUSED_OFF = threading.local()    # per host thread (the request-queue worker's retry must not reroute the main thread's searches)


def knn_fused_on() -> bool:
    return os.environ.get("KNNSVC_KNN_FUSED", "1") != "0" and not getattr(_FUSED_OFF, "on", False)


class fused_off:
    """Context: every search inside takes the dot-matrix route (the retry after a candidate-buffer overflow)."""
    def __enter__(self):
        self.prev = getattr(_FUSED_OFF, "on", False); _FUSED_OFF.on = True
    def __exit__(self, *a):
        _FUSED_OFF.on = self.prev


class KnnOverflow(KnnSvcError):
    """The fused kNN route met a query row with more candidates than its buffer holds: the search has to be repeated on the
    dot-matrix route (``with ops.fused_off(): ...``).  Not an error of the data — many near-identical pool rows do it."""


def _knn_p_cap(dim: int) -> int:
    """Most fp32 rows (a multiple of 128) of one buffer resource."""
    return (KNN_RSRC_BYTES - 1) // (dim * 4) // 128 * 128


def knn_pool_chunks(npool: int, dim: int):
    """The f16x2 routes' pool chunk plan: [(first row, end row), ...] — balanced chunks (no tail shorter than k) of at most
    p_cap rows, so that every buffer resource of a chunk (fp32 rows, split image) stays below KNN_RSRC_BYTES."""
    n_chunks = max(1, -(-npool // _knn_p_cap(dim)))
    p_rows = -(-npool // n_chunks)
    return [(p0, min(npool, p0 + p_rows)) for p0 in range(0, npool, p_rows)]


def knn_epochs(nq: int, npc: int, blocks: int = 256):
    """Column-tile ranges [(t0, t1), ...] (tiles of 256 pool rows) of the fused route's epochs.  The first epoch has no
    thresholds (every tile bounds its rows itself and lets ~45 of its 256 columns per row through), so it is about ONE round
    of workgroups — enough columns for a useful k-th distance (at least 4 tiles), few enough for the candidate buffer; every
    later epoch multiplies the rows seen by KNN_EPOCH_GROWTH: a row's survivors per epoch are ~k x (new rows / rows seen), and
    each epoch boundary costs one refine launch and the tail of a round.  A last epoch much smaller than its predecessor is
    merged into it."""
    gx, gy = -(-nq // 256), -(-npc // 256)
    e0 = min(gy, max(4, min(KNN_COLD_TILES_MAX, max(1, blocks) // gx)))
    out, c = [(0, e0)], e0
    while c < gy:
        nxt = min(gy, c * KNN_EPOCH_GROWTH)
        if gy - nxt < (nxt - c) // 2:
            nxt = gy
        out.append((c, nxt)); c = nxt
    return out


# What knn_plan returns.  KnnBlock: query rows [q0, q0 + m) of one pool chunk; fused route: the block's ``epochs`` (knn_epochs) and
# the int32 words it needs zeroed, ``fill``: candidate counts [m] | the first epoch's workspace: row bounds [m], per-half-tile
# bounds [2 gy0][m] (the tiles' exchange, knn.hip), arrival counters [gx] one cache line each.  KnnChunkPlan: pool rows
# [p0, p1), their route, ``npad`` = rows of their split image = columns of their dot matrix, the query blocks.  KnnPlan:
# ``fill_words``: the first-epoch workspace that rides in the search's one fill (0: every block zeroes its own).
KnnBlock = namedtuple("KnnBlock", "q0 m epochs fill")
KnnChunkPlan = namedtuple("KnnChunkPlan", "p0 p1 fused npad blocks")
KnnPlan = namedtuple("KnnPlan", "chunks fill_words")
# One chunk of a prepared pool: first row, fp32 rows (a view), their f16x2 image (npad rows), range slot.
KnnChunk = namedtuple("KnnChunk", "p0 rows image slot")


def knn_plan(nq: int, npool: int, dim: int, k: int, *, allow_fused=True, max_blocks=0, chunk_bounds=None) -> KnnPlan:
    """How an f16x2 search is cut up — integers only, nothing touches the device.  The pool in chunks (``chunk_bounds``: those
    of a prepared pool, else knn_pool_chunks); each chunk on the fused route (knnsvc_knn_screen + knnsvc_knn_refine) or the
    dot-matrix route (knnsvc_conv_gemm + knnsvc_knn_select); its queries in blocks so that the split image, the candidate
    buffer and the dot matrix each stay within KNN_RSRC_BYTES; a fused block in epochs.  ``fill_words`` is non-zero only where
    the search is ONE pool chunk, fused, in ONE query block: a second chunk or block must not inherit the first one's row
    bounds and arrival counters."""
    R = KNN_RSRC_BYTES
    fused_q = allow_fused and knn_fused_on() and nq >= KNN_FUSED_MIN_Q
    chunks = []
    for p0, p1 in (knn_pool_chunks(npool, dim) if chunk_bounds is None else chunk_bounds):
        npc = p1 - p0
        if npc < k:
            raise KnnSvcError("knn_topk: pool chunk smaller than k")
        # rows padded to a multiple of 4 (zero images): the dot-matrix GEMM runs on the 256x256 kernel, whose 16-byte epilogue
        # wants n % 4 == 0 — the padded columns' dots are never looked at (knn_select gets the true row count)
        npad = -(-npc // 4) * 4
        fused = fused_q and npc >= KNN_FUSED_MIN_P
        q_rows = (max(256, min(nq, (R // 4 - 1) // dim // 256 * 256, R // (KNN_FUSED_CAP * 8) // 256 * 256)) if fused else
                  max(128, min(nq, _knn_p_cap(dim), (R // 4) // max(npad, 1) // 128 * 128)))
        blocks = []
        for q0 in range(0, nq, q_rows):
            m = min(q_rows, nq - q0)
            ep = tuple(knn_epochs(m, npc, int(max_blocks) if max_blocks else 256)) if fused else ()
            blocks.append(KnnBlock(q0, m, ep, m * (2 + 2 * (ep[0][1] - ep[0][0])) + 32 * -(-m // 256) if fused else 0))
        chunks.append(KnnChunkPlan(p0, p1, fused, npad, tuple(blocks)))
    one = len(chunks) == 1 and chunks[0].fused and len(chunks[0].blocks) == 1
    return KnnPlan(tuple(chunks), chunks[0].blocks[0].fill if one else 0)


def knn_search_fill(nq: int, npool: int, dim: int, max_blocks: int = 0) -> int:
    """int32 words of the fused route's first-epoch workspace that knn_topk folds into its one fill (0: none): knn_plan's."""
    return knn_plan(nq, npool, dim, 1, max_blocks=max_blocks).fill_words


def prepare_knn_pool(pool, k=32, p_stats=None, plan=None):
    """Pre-split image of a pool for the two-kernel kNN route, reusable across searches against the same pool
    (dataset mode and prematch search one pool once per utterance): list of KnnChunk (first row, rows view, f16x2 image, range
    slot), cut where ``plan`` says (a search hands in its own; default: knn_plan's chunks for this pool).  The fp16 split
    needs a power-of-two pre-scale that fits the features' range; WavLM features have no a-priori bound (outlier channels),
    so the scale is derived ON THE DEVICE from max|pool| (knnsvc_absmax -> knnsvc_split_f16x2_dyn; the GEMM reads the same
    slot as w_absmax) — no host round trip, no fixed range.
    Returns None when the route does not apply (see knn_topk)."""
    _need(pool, name="knn.pool")
    npool, dim = pool.shape
    if not (knn_mode() == "f16x2" and dim % 32 == 0 and npool >= k and pool.is_contiguous()):
        return None
    chunks = []
    for p0, p1, _, npad, _ in (plan or knn_plan(0, npool, dim, k)).chunks:
        pc, npc = pool[p0:p1], p1 - p0
        slot = getattr(p_stats[0], "_slot", None) if p_stats is not None else None      # bound of the whole pool: fine for a chunk
        if slot is None:
            slot = absmax(pc)
        p2 = torch.empty(npad * (dim // 32) * 64, device=pool.device, dtype=torch.int16)
        if npad != npc:
            p2[npc * (dim // 32) * 64:].zero_()
        check(_lib.load().knnsvc_split_f16x2_dyn(_p(pc), npc, dim, _p(slot), _p(p2), _stream()), "split_pool")
        chunks.append(KnnChunk(p0, pc, p2, slot))
    return chunks


def knn_rescore_on() -> bool:
    """KNNSVC_KNN_RESCORE=0 (A/B aid): the lists keep the order of the screening distances (round 4's behaviour) instead of
    being re-scored from exact dot products (knnsvc_knn_rescore)."""
    return os.environ.get("KNNSVC_KNN_RESCORE", "1") != "0"


def knn_guard(dim: int, mode: str = "f16x2") -> float:
    """Guard band of a search's wide lists (csrc/knn.hip: KNN_GUARD, knn_guard_fp32): the f16x2 routes keep KNN_GUARD, the
    fp32-MFMA tile route (KNNSVC_KNN=fp32), whose screening error grows with dim, 5e-7 sqrt(dim) and at least KNN_GUARD."""
    return KNN_GUARD if mode != "fp32" else max(KNN_GUARD, 5.0e-7 * math.sqrt(dim))


# What every launch of an f16x2 search reads.  ``q2`` / ``q_slot``: the queries' f16x2 image and range slot (_knn_search); ``pn`` /
# ``ps`` / ``mask`` / ``idx_offset`` count pool rows from the pool's first row — or, in the form the executors get (_knn_search), from a chunk's.
_KnnSearch = namedtuple("_KnnSearch", "q qn qs pn ps k idx_offset mask flag max_blocks q2 q_slot", defaults=(None, None))


def _knn_rescore(s, c, q0, m, wide, idx_out, dist_out):
    """wide [m, 64] int64 keys of query rows [q0, q0 + m) -> their exact top-k (rows q0.. of idx_out / dist_out [nq, k])."""
    check(_lib.load().knnsvc_knn_rescore(_p(wide), m, s.k, _p(s.q[q0:]), _p(s.qn[q0:]), _p(s.qs[q0:]), _p(c.rows), _p(s.pn), _p(s.ps),
                                         c.rows.shape[0], s.q.shape[1], s.idx_offset, s.mask[0], s.mask[1], 1 if knn_rescore_on() else 0,
                                         _p(idx_out[q0:]), _p(dist_out[q0:]), _stream()), "knn_rescore")


def _knn_dot_chunk(s, c, plan, idx_out, dist_out):
    """One pool chunk through the dot matrix: per query block knnsvc_conv_gemm (fixed_tile = 2, pool rows = pre-split
    "weights") + knnsvc_knn_select.  ``s`` is chunk-local."""
    dev, dim, npc = s.q.device, s.q.shape[1], c.rows.shape[0]
    for q0, m, _, _ in plan.blocks:
        dots = torch.empty(m, plan.npad, device=dev, dtype=torch.float32)
        conv_gemm(s.q2[q0:q0 + m], c.rows, dots, m=m, n=plan.npad, cin=dim, w2=c.image, x_split=True, x_absmax=s.q_slot,
                  w_absmax=c.slot, fixed_tile=2)    # a shard / a query set of any size gives the whole search's distance bits
        wide = torch.empty(m, KNN_WIDE, device=dev, dtype=torch.int64)
        check(_lib.load().knnsvc_knn_select(_p(dots), plan.npad, _p(s.qn[q0:]), _p(s.qs[q0:]), m, _p(s.pn), _p(s.ps), npc, s.k,
                                            s.mask[0], s.mask[1], _p(wide), _p(s.flag), _stream()), "knn_select")
        _knn_rescore(s, c, q0, m, wide, idx_out, dist_out)


def _knn_fused_chunk(s, c, plan, idx_out, dist_out, zeros=None):
    """One pool chunk without a [nq, np] dot matrix: the chunk's rows in epochs (knn_epochs), each one knnsvc_knn_screen (the
    first without thresholds, the later ones against the row's k-th key so far) + one knnsvc_knn_refine (list so far + the new
    candidates -> list, next thresholds).  A row with more survivors than the candidate buffer holds (pathological data: e.g.
    thousands of bit-identical pool rows inside the first epoch) sets bit 1 of the flag; nothing here reads it.  ``s`` is
    chunk-local; ``zeros``: the block's ``fill`` words, already zeroed as part of the search's ONE fill (knn_plan: fill_words)."""
    lib = _lib.load()
    dev, dim, npc = s.q.device, s.q.shape[1], c.rows.shape[0]
    row_u16 = (dim // 32) * 64                                     # int16 elements of one pool row in the split image
    for q0, m, epochs, fill in plan.blocks:
        zeroed = zeros if zeros is not None else torch.zeros(fill, device=dev, dtype=torch.int32)
        cnt, bound = zeroed[:m], zeroed[m:]
        cand = torch.empty(m * KNN_FUSED_CAP * 2, device=dev, dtype=torch.int32)
        wide = torch.empty(m, KNN_WIDE, device=dev, dtype=torch.int64)       # the rows' wide lists, handed from epoch to epoch
        thr = torch.empty(m, device=dev, dtype=torch.float32)
        thr_idx = torch.empty(m, device=dev, dtype=torch.int64)
        for e, (t0, t1) in enumerate(epochs):
            c0, c1 = t0 * 256, min(t1 * 256, npc)
            last = e == len(epochs) - 1
            # both kernels OR their bits straight into the search's flag (bit 0: NaN distance, bit 1: candidate-buffer overflow
            # or a short list): no glue kernels between the launches
            check(lib.knnsvc_knn_screen(_p(s.q2[q0:]), _p(s.q_slot), _p(s.qn[q0:]), _p(s.qs[q0:]), m, _p(c.image[c0 * row_u16:]), _p(c.slot),
                                        _p(s.pn[c0:]), _p(s.ps[c0:]), c1 - c0, dim, _p(thr) if e else _p(None), _p(thr_idx) if e else _p(None),
                                        s.mask[0], s.mask[1], c0, _p(cnt), _p(cand), KNN_FUSED_CAP, _p(None) if e else _p(bound), _p(s.flag),
                                        int(s.max_blocks), _stream()), "knn_screen")
            if KNN_DEBUG_COUNTS is not None:           # tools/knn_prof.py: survivors per row and epoch (a clone: refine resets the counts)
                KNN_DEBUG_COUNTS.append((e, cnt.clone()))
            check(lib.knnsvc_knn_refine(_p(cnt), _p(cand), KNN_FUSED_CAP, m, s.k, _p(None) if e else _p(bound), 1 if e else 0, _p(wide),
                                        _p(None) if last else _p(thr), _p(None) if last else _p(thr_idx), 1 if last else 0, _p(s.flag),
                                        _stream()), "knn_refine")
        # the candidates' order came from the screening products; the order that goes out comes from exact ones
        _knn_rescore(s, c, q0, m, wide, idx_out, dist_out)


def _knn_search(s, pool, prepared, plan, zeros=None):
    """``plan`` (knn_plan) carried out: q.p^T on the f16x2 matrix-core loop (Gemm2QuadS), then the reference's distance formula
    + selection, on two routes over the SAME dot-product bits (both sum over K in the 16x16x32 grouping, whatever the sizes).
    Both operands are scaled by device-chosen powers of two (range slots, see prepare_knn_pool) — exact, so the dots do not
    depend on the scale.  Pool chunks are folded with knnsvc_knn_merge.  ``s.flag``: bit 0 = NaN distance, bit 1 = the fused
    route's candidate buffer overflowed (the results are then NOT valid: knn_topk / raise_if_nan turn it into a retry on the
    dot-matrix route) — read by the caller, never here: no host synchronisation inside a search.  ``zeros``: plan.fill_words
    zeroed words."""
    q, k, dev = s.q, s.k, s.q.device
    nq, dim = q.shape
    # the queries are split once into the A2 layout (the weight-split kernel writes exactly that image)
    q_slot = getattr(s.qn, "_slot", None)
    if q_slot is None:
        q_slot = absmax(q)
    q2 = torch.empty(nq, dim, device=dev, dtype=torch.float32)
    check(_lib.load().knnsvc_split_f16x2_dyn(_p(q), nq, dim, _p(q_slot), _p(q2), _stream()), "split_queries")
    s = s._replace(q2=q2, q_slot=q_slot)
    parts = []
    for c, cp in zip(prepared if prepared is not None else prepare_knn_pool(pool, k, (s.pn, s.ps), plan), plan.chunks):
        idx = torch.empty(nq, k, device=dev, dtype=torch.int64)
        dist = torch.empty(nq, k, device=dev, dtype=torch.float32)
        KNN_ROUTE_COUNTS["chunks"] += 1; KNN_ROUTE_COUNTS["fused" if cp.fused else "dot"] += 1
        # the search as this chunk sees it — the one place the chunk-local views are formed
        loc = s._replace(pn=s.pn[c.p0:], ps=s.ps[c.p0:], mask=(s.mask[0] - c.p0, s.mask[1] - c.p0), idx_offset=s.idx_offset + c.p0)
        if cp.fused:
            _knn_fused_chunk(loc, c, cp, idx, dist, zeros)
        else:
            _knn_dot_chunk(loc, c, cp, idx, dist)
        parts.append((idx, dist))
    return parts[0] if len(parts) == 1 else knn_merge(torch.stack([d for _, d in parts]), torch.stack([i for i, _ in parts]))


def knn_topk(q, pool, k=32, idx_offset=0, q_stats=None, p_stats=None, check_nan=True, return_flag=False, mask=None,
             prepared=None, max_blocks=0):
    """Ascending cosine-distance top-k of each q row among pool rows -> (idx int64 [nq,k], dist f32 [nq,k]).
    ``mask`` = (lo, hi): pool rows [lo, hi) compete at distance exactly 1 (self-matching of per_spk_extract,
    ddsp_prematch_dataset.py:1606-1607).
    ``check_nan=True``: the flag is read here (one sync); a NaN raises, a candidate-buffer overflow of the fused route repeats the
    search on the dot-matrix route.  ``check_nan=False, return_flag=True``: nothing is read; the caller hands the flag to
    ``raise_if_nan`` once everything is enqueued (KnnOverflow -> it repeats the work with ``fused_off()``).
    ``prepared``: prepare_knn_pool's chunks of this pool; the search is then planned on their bounds.
    ``max_blocks``: grid cap of the persistent screening kernel (0 = the whole chip)."""
    mask = (0, 0) if mask is None else (int(mask[0]), int(mask[1]))
    _need(q, name="knn.q"); _need(pool, name="knn.pool")
    if not (q.is_contiguous() and pool.is_contiguous()):
        raise KnnSvcError("knn_topk: q and pool must be contiguous")
    lib = _lib.load()
    nq, dim = q.shape
    npool = pool.shape[0]
    f16 = knn_mode() == "f16x2" and dim % 32 == 0 and npool >= k and nq > 0 and 1 <= k <= 32
    # ONE fill for everything a search needs zeroed — its flag, the two operands' range slots and (one fused block over a pool
    # that is not prepared: plan.fill_words) the candidate counts + first-epoch workspace: four tiny fill launches were ~5 us
    # each in front of a 0.4 ms search
    flag = zeros = None
    if f16:
        bounds = None if prepared is None else [(c.p0, c.p0 + c.rows.shape[0]) for c in prepared]
        plan = knn_plan(nq, npool, dim, k, max_blocks=max_blocks, chunk_bounds=bounds)
        nz = plan.fill_words if prepared is None else 0
        zbuf = torch.zeros(64 + 2 * SLOT_W + nz, device=q.device, dtype=torch.int32)
        flag = zbuf[:1]
        sl_q, sl_p = zbuf[64:64 + SLOT_W].view(torch.float32), zbuf[64 + SLOT_W:64 + 2 * SLOT_W].view(torch.float32)
        zeros = zbuf[64 + 2 * SLOT_W:] if nz else None
    qn, qs = q_stats if q_stats is not None else row_norms(q, sl_q if f16 else None)
    pn, ps = p_stats if p_stats is not None else row_norms(pool, sl_p if f16 else None)
    if f16:
        s = _KnnSearch(q, qn, qs, pn, ps, k, idx_offset, mask, flag, max_blocks)
        idx, dist = _knn_search(s, pool, prepared, plan, zeros)
        if check_nan:
            try:
                raise_if_nan(flag)
            except KnnOverflow:
                flag.zero_()
                idx, dist = _knn_search(s, pool, prepared, knn_plan(nq, npool, dim, k, allow_fused=False, chunk_bounds=bounds))
                raise_if_nan(flag)
        return (idx, dist, flag) if return_flag else (idx, dist)
    ws_bytes = lib.knnsvc_knn_workspace_bytes(nq, npool, k)
    ws = torch.empty(max(ws_bytes, 8), device=q.device, dtype=torch.uint8)
    idx = torch.empty(nq, k, device=q.device, dtype=torch.int64)
    dist = torch.empty(nq, k, device=q.device, dtype=torch.float32)
    flag = torch.zeros(1, device=q.device, dtype=torch.int32)
    check(lib.knnsvc_knn_topk(_p(q), _p(qn), _p(qs), nq, _p(pool), _p(pn), _p(ps), npool, dim, k, idx_offset, mask[0], mask[1],
                              _p(idx), _p(dist), _p(ws), ws_bytes, _p(flag), 1 if knn_rescore_on() else 0, _stream()), "knn_topk")
    if check_nan:
        raise_if_nan(flag)
    return (idx, dist, flag) if return_flag else (idx, dist)


def retry_on_overflow(fn):
    """fn() with deferred flag checks inside; if one of them reports a candidate-buffer overflow of the fused kNN route, the
    whole of fn is repeated with every search on the dot-matrix route.  (fn must be repeatable: it recomputes its outputs.)"""
    try:
        return fn()
    except KnnOverflow:
        KNN_ROUTE_COUNTS["overflow_retries"] = KNN_ROUTE_COUNTS.get("overflow_retries", 0) + 1
        with fused_off():
            return fn()


def raise_if_nan(flag):
    """Host check of a search's device flag (one sync).  Bit 0: a NaN distance — the reference prints 'containing nan' and
    sys.exit()s inside fast_cosine_dist (lib_ongaku_test.py:166-169).  Bit 1: KnnOverflow.  Callers may defer this check to
    the end of a launch sequence so that it does not split the stream."""
    v = int(flag.item())
    if v & 1:
        raise KnnSvcError("containing nan")
    if v & KNN_OVERFLOW:
        raise KnnOverflow("fused kNN route: candidate buffer overflow (repeat with ops.fused_off())")


def reload_knobs() -> None:
    """Re-read the dispatchers' A/B switches (KNNSVC_QUAD, KNNSVC_QUAD_EPI, KNNSVC_EPILOGUE, KNNSVC_WIN*, KNNSVC_GEMM_SMALL,
    KNNSVC_ATTENTION, KNNSVC_CONV0_RP, KNNSVC_CONV0_SUBS) from the environment: the library reads them once, when a dispatcher
    first looks at them (csrc/common.h: KnKnobs)."""
    check(_lib.load().knnsvc_reload_knobs(), "reload_knobs")


def knn_merge(part_dist, part_idx):
    """[parts, nq, k] per-shard lists (global indices) -> merged (idx, dist)."""
    parts, nq, k = part_dist.shape
    idx = torch.empty(nq, k, device=part_dist.device, dtype=torch.int64)
    dist = torch.empty(nq, k, device=part_dist.device, dtype=torch.float32)
    check(_lib.load().knnsvc_knn_merge(_p(part_dist.contiguous()), _p(part_idx.contiguous()), parts, nq, k,
                                       _p(idx), _p(dist), _stream()), "knn_merge")
    return idx, dist


# ------------------------------------------------------------------ neighbour post-processing
def log_f0_median(f0):
    """-> tensor [2] on device: (lower median of log f0 over voiced frames, voiced count)."""
    _need(f0, name="f0")
    res = torch.empty(2, device=f0.device, dtype=torch.float32)
    ws = torch.empty(f0.numel(), device=f0.device, dtype=torch.float32)
    check(_lib.load().knnsvc_log_f0_median(_p(f0), f0.numel(), _p(res), _p(ws), _stream()), "log_f0_median")
    return res


def shift_f0(f0, qmed, pmed):
    out = torch.empty_like(f0)
    check(_lib.load().knnsvc_shift_f0(_p(f0), f0.numel(), _p(qmed), _p(pmed), _p(out), _stream()), "shift_f0")
    return out


def f0_rerank(nn_idx, shifted_f0, pool_f0):
    _need(nn_idx, torch.int64, "nn_idx")
    out = torch.empty_like(nn_idx)
    nq, k = nn_idx.shape
    check(_lib.load().knnsvc_f0_rerank(_p(nn_idx), nq, k, _p(shifted_f0), _p(pool_f0), _p(out), _stream()), "f0_rerank")
    return out


def _topk_of(name, idx):
    """k of an [rows, k] neighbour table as the match-stage kernels take it (1..8: one K-templated kernel per stage; 4 also has
    fast paths, which KNNSVC_MATCH_GENERIC_K=1 skips)."""
    if idx.dim() != 2 or not 1 <= idx.shape[1] <= 8:
        raise KnnSvcError(f"{name}: idx must be [rows, k] with 1 <= k <= 8, got {tuple(idx.shape)}")
    return int(idx.shape[1])


def concat_reselect(idx4, q, q_norm, pool, p_norm, shifted_f0=None, pool_f0=None, concat_weight=0.2):
    """``idx4`` [nq, k]: k = 4 is the specialised entry point, any other k in 1..8 the one-segment case of the k-taking one."""
    _need(idx4, torch.int64, "idx4")
    if _topk_of("concat_reselect", idx4) != 4:
        return concat_reselect_seg(idx4, [0, idx4.shape[0]], q, q_norm, pool, p_norm, shifted_f0, pool_f0, concat_weight)
    idx4 = idx4.contiguous()
    out = torch.empty_like(idx4)
    use_f0 = shifted_f0 is not None
    check(_lib.load().knnsvc_concat_reselect(_p(idx4), _p(q), _p(q_norm), q.shape[0], _p(pool), _p(p_norm),
                                             pool.shape[0], q.shape[1], _p(shifted_f0), _p(pool_f0), 1 if use_f0 else 0,
                                             float(concat_weight), _p(out), _stream()), "concat_reselect")
    return out


ADAM_FORCED_ITERS = None     # measurement aid (bench.py "value_long_adam"): run exactly this many iterations per loop


def _smooth_args(name, idx4, pool, max_iter, row_scale):
    """The checks smooth_weights and smooth_weights_seg share -> (contiguous idx4, max_iter as the library takes it)."""
    if ADAM_FORCED_ITERS:
        max_iter = -int(ADAM_FORCED_ITERS)
    _need(idx4, torch.int64, "idx4"); _need(pool, name="pool")
    if row_scale is not None:
        _need(row_scale, name="row_scale")
        if tuple(row_scale.shape) != tuple(idx4.shape) or not row_scale.is_contiguous():
            raise KnnSvcError(f"{name}: row_scale must be a contiguous [rows,k] tensor")
    return idx4.contiguous(), int(max_iter)


def smooth_weights(idx4, pool, scale, max_iter=100000, return_iters=False, row_scale=None):
    """``row_scale`` [nq,4]: the amp_ratio of compute_weight_with_amp (ddsp_prematch_dataset.py:684-804)."""
    if _topk_of("smooth_weights", idx4) != 4:
        return smooth_weights_seg(idx4, [0, idx4.shape[0]], pool, scale, max_iter, return_iters, row_scale)
    idx4, max_iter = _smooth_args("smooth_weights", idx4, pool, max_iter, row_scale)
    lib = _lib.load()
    nq = idx4.shape[0]
    npool, dim = pool.shape
    ws_bytes = lib.knnsvc_smooth_workspace_bytes(nq)
    ws = torch.empty(ws_bytes, device=pool.device, dtype=torch.uint8)
    w = torch.empty(nq, 4, device=pool.device, dtype=torch.float32)
    iters = torch.zeros(1, device=pool.device, dtype=torch.int32)
    check(lib.knnsvc_smooth_weights(_p(idx4), nq, _p(pool), npool, dim, pool.stride(0), float(scale), _p(row_scale), max_iter,
                                    _p(w), _p(iters), _p(ws), ws_bytes, _stream()), "smooth_weights")
    return (w, iters) if return_iters else w


# ------------------------------------------------------------------ the same stages for several stacked sequences
MAX_SEGMENTS = 64            # KNNSVC_MAX_SEGMENTS


def _seg_chunks(seg):
    """``seg``: Python list of row offsets [0, ..., total] of the stacked sequences -> [(first segment, row offset, host table)]
    in runs of at most MAX_SEGMENTS segments (one library call each; the table is read by the call, not kept)."""
    seg = [int(v) for v in seg]
    if len(seg) < 2:
        raise KnnSvcError("segment table: need at least one segment")
    out = []
    for a in range(0, len(seg) - 1, MAX_SEGMENTS):
        b = min(a + MAX_SEGMENTS, len(seg) - 1)
        out.append((a, seg[a], (C.c_int64 * (b - a + 1))(*[v - seg[a] for v in seg[a:b + 1]])))
    return out


class Segments:
    """Row offsets prepared once (the host tables of _seg_chunks) for any number of *_seg calls; each takes the Python list or this."""

    def __init__(self, seg):
        self.chunks, self.n, self.total, self.offsets = _seg_chunks(seg), len(seg) - 1, int(seg[-1]), list(seg)

    def __iter__(self):
        return iter(self.offsets)

    @classmethod
    def of_lengths(cls, lens):
        """The table of sequences of ``lens`` rows stacked one after the other."""
        seg = [0]
        for n in lens:
            seg.append(seg[-1] + int(n))
        return cls(seg)


def _segments(seg, name, *stacked):
    """``seg`` as Segments, checked against the row count of the ``stacked`` tensors."""
    seg = seg if isinstance(seg, Segments) else Segments(seg)
    for t in stacked:
        if t.shape[0] != seg.total:
            raise KnnSvcError(f"{name}: {t.shape[0]} rows for a segment table that ends at {seg.total}")
    return seg


def log_f0_median_seg(f0, seg):
    """-> tensor [n_seg, 2]: ``log_f0_median`` of every segment."""
    _need(f0, name="f0"); seg = _segments(seg, "log_f0_median_seg", f0)
    f0 = f0.contiguous()
    res = torch.empty(seg.n, 2, device=f0.device, dtype=torch.float32)
    ws = torch.empty(f0.numel(), device=f0.device, dtype=torch.float32)
    for a, r0, tab in seg.chunks:
        check(_lib.load().knnsvc_log_f0_median_seg(_p(f0[r0:]), tab, len(tab) - 1, _p(res[a:]), _p(ws[r0:]), _stream()), "log_f0_median_seg")
    return res


F0_SHIFT_MEDIAN, F0_SHIFT_OCTAVE, F0_SHIFT_SEMITONE, F0_SHIFT_NONE = range(4)      # KNNSVC_F0_SHIFT_*


def shift_f0_seg(f0, seg, qmed, pmed, modes=None, transposes=None, return_shift=False):
    """``qmed`` [n_seg, 2] from log_f0_median_seg, ``pmed`` [2] -> shifted f0 of the stacked rows.
    ``modes`` (per segment: 0 median, 1 octave, 2 semitone, 3 none) and ``transposes`` (per segment, semitones): the interval
    is then chosen per segment on the device (knnsvc_shift_f0_seg_mode; include/knnsvc_hip.h "Pitch control"); with both None
    this is the median shift through knnsvc_shift_f0_seg (the same kernel with median / 0).  ``return_shift``: -> (shifted, [n_seg] applied interval in
    semitones, on the device)."""
    return _shift_f0_seg("shift_f0_seg", f0, seg, qmed, pmed, modes, transposes, return_shift)


def _shift_f0_seg(fn, f0, seg, qmed, pmed, modes, transposes, return_shift, weights=None):
    """``shift_f0_seg`` and, with ``weights`` (``pmed`` is then its ``pmeds``), ``shift_f0_seg_blend``."""
    _need(f0, name="f0"); seg = _segments(seg, fn, f0)
    _need(qmed, name="qmed"); _need(pmed, name="pmed" if weights is None else "pmeds")
    if qmed.numel() != 2 * seg.n or not qmed.is_contiguous():
        raise KnnSvcError(f"{fn}: qmed must be a contiguous [{seg.n}, 2] tensor, got {tuple(qmed.shape)}")
    if weights is not None:
        if pmed.dim() != 2 or pmed.shape[1] != 2 or not pmed.is_contiguous():
            raise KnnSvcError(f"{fn}: pmeds must be a contiguous [n_voices, 2] tensor, got {tuple(pmed.shape)}")
        nv = int(pmed.shape[0])
        rows = _blend_rows(fn, weights, seg.n, nv)
    for name, t in (("modes", modes), ("transposes", transposes)):
        if t is not None and len(t) != seg.n:
            raise KnnSvcError(f"{fn}: {len(t)} {name} for {seg.n} segments")
    f0 = f0.contiguous()
    out = torch.empty_like(f0)
    semis = torch.empty(seg.n, device=f0.device, dtype=torch.float32) if return_shift else None
    plain = weights is None and modes is None and transposes is None and not return_shift
    lib = _lib.load()
    for a, r0, tab in seg.chunks:
        n = len(tab) - 1
        if plain:
            check(lib.knnsvc_shift_f0_seg(_p(f0[r0:]), tab, n, _p(qmed[a:]), _p(pmed), _p(out[r0:]), _stream()), "shift_f0_seg")
            continue
        mt = None if modes is None else (C.c_int32 * n)(*[int(m) for m in modes[a:a + n]])
        tt = None if transposes is None else (C.c_float * n)(*[float(t) for t in transposes[a:a + n]])
        dst = (_p(out[r0:]), _p(semis[a:]) if return_shift else None, _stream())
        if weights is None:
            check(lib.knnsvc_shift_f0_seg_mode(_p(f0[r0:]), tab, n, mt, tt, _p(qmed[a:]), _p(pmed), *dst), "shift_f0_seg_mode")
        else:
            wt = (C.c_double * (n * nv))(*[w for row in rows[a:a + n] for w in row])
            check(lib.knnsvc_shift_f0_seg_blend(_p(f0[r0:]), tab, n, mt, tt, _p(qmed[a:]), _p(pmed), nv, wt, *dst), fn)
    return (out, semis) if return_shift else out


def concat_reselect_seg(idx4, seg, q, q_norm, pool, p_norm, shifted_f0=None, pool_f0=None, concat_weight=0.2):
    """``concat_reselect`` of every segment of the stacked rows: one workgroup per segment in one launch."""
    _need(idx4, torch.int64, "idx4"); seg = _segments(seg, "concat_reselect_seg", idx4, q)
    k = _topk_of("concat_reselect_seg", idx4)
    idx4 = idx4.contiguous()
    out = torch.empty_like(idx4)
    use_f0 = shifted_f0 is not None
    lib = _lib.load()
    for a, r0, tab in seg.chunks:
        tail = (tab, len(tab) - 1, _p(pool), _p(p_norm), pool.shape[0], q.shape[1], _p(shifted_f0[r0:]) if use_f0 else _p(None),
                _p(pool_f0), 1 if use_f0 else 0, float(concat_weight), _p(out[r0:]), _stream())
        if k == 4:
            check(lib.knnsvc_concat_reselect_seg(_p(idx4[r0:]), _p(q[r0:]), _p(q_norm[r0:]), *tail), "concat_reselect_seg")
        else:
            check(lib.knnsvc_concat_reselect_seg_k(_p(idx4[r0:]), k, _p(q[r0:]), _p(q_norm[r0:]), *tail), "concat_reselect_seg_k")
    return out


def smooth_weights_seg(idx4, seg, pool, scale, max_iter=100000, return_iters=False, row_scale=None):
    """``smooth_weights`` of every segment of the stacked rows -> w [total, k] (and iters [n_seg]); k = idx4.shape[1] in 1..8."""
    idx4, max_iter = _smooth_args("smooth_weights_seg", idx4, pool, max_iter, row_scale)
    seg = _segments(seg, "smooth_weights_seg", idx4)
    k = _topk_of("smooth_weights_seg", idx4)
    lib = _lib.load()
    npool, dim = pool.shape
    w = torch.empty(idx4.shape[0], k, device=pool.device, dtype=torch.float32)
    iters = torch.zeros(seg.n, device=pool.device, dtype=torch.int32)
    for a, r0, tab in seg.chunks:
        ws_bytes = lib.knnsvc_smooth_seg_workspace_bytes(tab, len(tab) - 1) if k == 4 else \
            lib.knnsvc_smooth_seg_workspace_bytes_k(tab, len(tab) - 1, k)
        ws = torch.empty(ws_bytes, device=pool.device, dtype=torch.uint8)
        tail = (tab, len(tab) - 1, _p(pool), npool, dim, pool.stride(0), float(scale), _p(row_scale[r0:]) if row_scale is not None else _p(None),
                max_iter, _p(w[r0:]), _p(iters[a:]), _p(ws), ws_bytes, _stream())
        if k == 4:
            check(lib.knnsvc_smooth_weights_seg(_p(idx4[r0:]), *tail), "smooth_weights_seg")
        else:
            check(lib.knnsvc_smooth_weights_seg_k(_p(idx4[r0:]), k, *tail), "smooth_weights_seg_k")
    return (w, iters) if return_iters else w


def time_scale_seg(x, f0, seg, out_frames, inv_scales, out=None):
    """The stacked sequences of ``seg`` re-timed along the frame axis (knnsvc_time_scale_seg; include/knnsvc_hip.h "Time scale"
    is the specification): segment s gets ``out_frames[s]`` >= 1 rows, read at the source positions ``inv_scales[s]`` (= 1 /
    scale factor, finite and > 0) spaces.  ``x`` [total, dim] features and ``f0`` [total], either may be None -> (x_out, f0_out)
    with None for None.  The caller decides the lengths and the scales (matching.duration_plan).  ``out``: (x_out, f0_out)
    buffers to write into instead of new ones.  Enqueue only: nothing is read back."""
    given = [(n, t) for n, t in (("x", x), ("f0", f0)) if t is not None]
    if not given:
        raise KnnSvcError("time_scale_seg: neither features nor f0 given")
    for n, t in given:
        _need(t, name=n)
        if not t.is_contiguous():
            raise KnnSvcError(f"time_scale_seg: {n} must be contiguous")
    if x is not None and (x.dim() != 2 or x.shape[1] < 1):
        raise KnnSvcError(f"time_scale_seg: x must be [rows, dim], got {tuple(x.shape)}")
    if f0 is not None and f0.dim() != 1:
        raise KnnSvcError(f"time_scale_seg: f0 must be [rows], got {tuple(f0.shape)}")
    seg = _segments(seg, "time_scale_seg", *[t for _, t in given])
    if len(out_frames) != seg.n or len(inv_scales) != seg.n:
        raise KnnSvcError(f"time_scale_seg: {len(out_frames)} out_frames and {len(inv_scales)} inv_scales for {seg.n} segments")
    for s, n in enumerate(out_frames):
        if isinstance(n, bool) or int(n) != n or int(n) < 1:
            raise KnnSvcError(f"time_scale_seg: segment {s}: out_frames must be an integer >= 1, got {n!r}")
    cs = [float(c) for c in inv_scales]
    for s, c in enumerate(cs):
        if not (math.isfinite(c) and c > 0):
            raise KnnSvcError(f"time_scale_seg: segment {s}: inv_scale must be finite and > 0, got {inv_scales[s]!r}")
    oseg = Segments.of_lengths(out_frames)
    dev = given[0][1].device
    dim = 0 if x is None else int(x.shape[1])
    xo, fo = out if out is not None else (None, None)
    if x is not None and xo is None:
        xo = torch.empty(oseg.total, dim, device=dev, dtype=torch.float32)
    if f0 is not None and fo is None:
        fo = torch.empty(oseg.total, device=dev, dtype=torch.float32)
    for n, t, shape in (("x_out", xo, (oseg.total, dim)), ("f0_out", fo, (oseg.total,))):
        if (t is None) != ((x if n == "x_out" else f0) is None):
            raise KnnSvcError(f"time_scale_seg: {n} given without its input, or the reverse")
        if t is not None:
            _need(t, name=n)
            if tuple(t.shape) != shape or not t.is_contiguous():
                raise KnnSvcError(f"time_scale_seg: {n} must be a contiguous {shape} tensor, got {tuple(t.shape)}")
    lib = _lib.load()
    # a chunk of at most MAX_SEGMENTS segments has TWO row offsets: where its rows start in the input and in the output
    for (a, r0, tab), (_a, o0, otab) in zip(seg.chunks, oseg.chunks):
        n = len(tab) - 1
        check(lib.knnsvc_time_scale_seg(_p(x[r0:]) if x is not None else _p(None), dim, _p(f0[r0:]) if f0 is not None else _p(None),
                                        tab, otab, (C.c_double * n)(*cs[a:a + n]), n, _p(xo[o0:]) if x is not None else _p(None),
                                        _p(fo[o0:]) if f0 is not None else _p(None), _stream()), "time_scale_seg")
    return xo, fo


def time_scale(x, f0, out_frames, inv_scale):
    """``time_scale_seg`` of one sequence -> (x_out [out_frames, dim] or None, f0_out [out_frames] or None)."""
    rows = (x if x is not None else f0).shape[0] if (x is not None or f0 is not None) else 0
    return time_scale_seg(x, f0, [0, int(rows)], [out_frames], [inv_scale])


BLEND_MAX_VOICES = 4         # KNNSVC_BLEND_MAX_VOICES


def _blend_rows(name, weights, n_seg, n_voices):
    """``weights`` ([n_seg][n_voices] numbers, one row per segment) as a list of tuples of floats, shape-checked; what the
    values have to satisfy (include/knnsvc_hip.h "Voice blend", point 4) the library checks before it launches."""
    if not 2 <= n_voices <= BLEND_MAX_VOICES:
        raise KnnSvcError(f"{name}: {n_voices} voices, expected 2..{BLEND_MAX_VOICES}")
    rows = [tuple(float(a) for a in row) for row in weights]
    if len(rows) != n_seg or any(len(r) != n_voices for r in rows):
        raise KnnSvcError(f"{name}: weights must be [{n_seg}][{n_voices}] (a row per segment), got {len(rows)} rows of "
                          f"{sorted(set(len(r) for r in rows))} entries")
    return rows


def blend_seg(xs, seg, weights, out=None):
    """The stacked rows of 2..4 voices (``xs``: contiguous [total, dim] fp32 tensors of one shape) mixed per segment with
    ``weights[s]`` (normalised by the caller: matching.resolve_blend) -> [total, dim] (knnsvc_blend_seg; include/knnsvc_hip.h
    "Voice blend" is the specification: fp64 products and sums in voice order, one rounding, a zero-weight voice not read, a
    single non-zero weight a copy).  ``out``: a buffer to write into.  One launch per 64 segments; enqueue only."""
    xs = list(xs)
    for v, x in enumerate(xs):
        _need(x, name=f"xs[{v}]")
        if x.dim() != 2 or x.shape[1] < 1 or not x.is_contiguous() or x.shape != xs[0].shape:
            raise KnnSvcError(f"blend_seg: xs[{v}] must be a contiguous [rows, dim] tensor of the voices' common shape, got {tuple(x.shape)}")
    if not xs:
        raise KnnSvcError("blend_seg: no voices")
    seg = _segments(seg, "blend_seg", *xs)
    rows = _blend_rows("blend_seg", weights, seg.n, len(xs))
    if out is None:
        out = torch.empty_like(xs[0])
    _need(out, name="out")
    if out.shape != xs[0].shape or not out.is_contiguous():
        raise KnnSvcError(f"blend_seg: out must be a contiguous {tuple(xs[0].shape)} tensor, got {tuple(out.shape)}")
    lib = _lib.load()
    nv, dim = len(xs), int(xs[0].shape[1])
    for a, r0, tab in seg.chunks:
        n = len(tab) - 1
        ptrs = (C.c_void_p * nv)(*[x[r0:].data_ptr() for x in xs])
        wt = (C.c_double * (n * nv))(*[w for row in rows[a:a + n] for w in row])
        check(lib.knnsvc_blend_seg(ptrs, nv, dim, tab, n, wt, _p(out[r0:]), _stream()), "blend_seg")
    return out


def shift_f0_seg_blend(f0, seg, qmed, pmeds, weights, modes=None, transposes=None, return_shift=False):
    """``shift_f0_seg`` towards a blend of voices: ``pmeds`` [n_voices, 2] (log_f0_median of each voice's pool, stacked) and
    ``weights`` [n_seg][n_voices] in place of the single ``pmed``; segment s is shifted towards the weighted mean of the voices'
    log medians, formed on the device (knnsvc_shift_f0_seg_blend; include/knnsvc_hip.h "Voice blend", point 3), after which modes
    and transposes act as in ``shift_f0_seg``."""
    return _shift_f0_seg("shift_f0_seg_blend", f0, seg, qmed, pmeds, modes, transposes, return_shift, weights)


def tune_f0_seg(f0, seg, tunings, return_notes=False):
    """Pitch correction of the stacked, shifted f0 (knnsvc_tune_f0_seg; include/knnsvc_hip.h "Pitch correction" is the
    specification).  ``tunings``: one options.Tuning or None (off) per segment -> the corrected f0, a new tensor; with
    ``return_notes`` -> (f0, int32 notes, -1 where nothing was corrected).  One launch per 64 segments; a run of 64 whose segments
    are all off is not launched (its rows are copied), and when every segment is off the INPUT TENSOR ITSELF comes back (notes:
    None) and nothing is launched, loaded or checked beyond the count.  Enqueue only."""
    n_seg = seg.n if isinstance(seg, Segments) else len(seg) - 1
    tunings = list(tunings)
    if len(tunings) != n_seg:
        raise KnnSvcError(f"tune_f0_seg: {len(tunings)} tunings for {n_seg} segments")
    live = [t is not None and t.on for t in tunings]
    if not any(live):
        return (f0, None) if return_notes else f0
    _need(f0, name="f0"); seg = _segments(seg, "tune_f0_seg", f0)
    if f0.dim() != 1:
        raise KnnSvcError(f"tune_f0_seg: f0 must be [rows], got {tuple(f0.shape)}")
    f0 = f0.contiguous()
    out = torch.empty_like(f0)
    notes = torch.empty(f0.numel(), device=f0.device, dtype=torch.int32) if return_notes else None
    lib = _lib.load()
    off = (0, 0.0, 1.0, math.log(440.0))
    for a, r0, tab in seg.chunks:
        n = len(tab) - 1
        r1 = r0 + tab[n]
        if not any(live[a:a + n]):
            out[r0:r1].copy_(f0[r0:r1])
            if return_notes:
                notes[r0:r1].fill_(-1)
            continue
        rows = [(t.mask, t.strength, t.alpha, t.log_ref) if on else off for t, on in zip(tunings[a:a + n], live[a:a + n])]
        ws_bytes = lib.knnsvc_tune_f0_workspace_bytes(tab[n], n)
        ws = torch.empty(ws_bytes, device=f0.device, dtype=torch.uint8)
        check(lib.knnsvc_tune_f0_seg(_p(f0[r0:]), tab, n, (C.c_int32 * n)(*[r[0] for r in rows]), (C.c_double * n)(*[r[1] for r in rows]),
                                     (C.c_double * n)(*[r[2] for r in rows]), (C.c_double * n)(*[r[3] for r in rows]), _p(out[r0:]),
                                     _p(notes[r0:]) if return_notes else None, _p(ws), ws_bytes, _stream()), "tune_f0_seg")
    return (out, notes) if return_notes else out


HARMONY_MAX_PARTS = 3        # KNNSVC_HARMONY_MAX_PARTS


def harmony_f0_seg(f0, seg, parts, return_notes=False):
    """The f0 contour of a harmony part from the lead's stacked final f0 (knnsvc_harmony_f0_seg; include/knnsvc_hip.h "Harmony
    voice" is the specification).  ``parts``: per segment None (off: the segment keeps its bits) or anything with ``mask`` /
    ``steps`` / ``alpha`` / ``log_ref`` (options.HarmonyShift) -> the part's f0, a new tensor; with ``return_notes`` -> (f0, int32
    notes of the part, -1 where nothing was moved).  One launch per 64 segments; a run of 64 whose segments are all off is not
    launched (its rows are copied), and when every segment is off the INPUT TENSOR ITSELF comes back (notes: None) and nothing is
    launched, loaded or checked beyond the count.  Enqueue only."""
    n_seg = seg.n if isinstance(seg, Segments) else len(seg) - 1
    parts = list(parts)
    if len(parts) != n_seg:
        raise KnnSvcError(f"harmony_f0_seg: {len(parts)} parts for {n_seg} segments")
    live = [p is not None and p.mask != 0 and p.steps != 0 for p in parts]
    if not any(live):
        return (f0, None) if return_notes else f0
    _need(f0, name="f0"); seg = _segments(seg, "harmony_f0_seg", f0)
    if f0.dim() != 1:
        raise KnnSvcError(f"harmony_f0_seg: f0 must be [rows], got {tuple(f0.shape)}")
    f0 = f0.contiguous()
    out = torch.empty_like(f0)
    notes = torch.empty(f0.numel(), device=f0.device, dtype=torch.int32) if return_notes else None
    lib = _lib.load()
    off = (0, 0, 1.0, math.log(440.0))
    for a, r0, tab in seg.chunks:
        n = len(tab) - 1
        r1 = r0 + tab[n]
        if not any(live[a:a + n]):
            out[r0:r1].copy_(f0[r0:r1])
            if return_notes:
                notes[r0:r1].fill_(-1)
            continue
        rows = [(int(p.mask), int(p.steps), float(p.alpha), float(p.log_ref)) if on else off for p, on in zip(parts[a:a + n], live[a:a + n])]
        ws_bytes = lib.knnsvc_tune_f0_workspace_bytes(tab[n], n)
        ws = torch.empty(ws_bytes, device=f0.device, dtype=torch.uint8)
        check(lib.knnsvc_harmony_f0_seg(_p(f0[r0:]), tab, n, (C.c_int32 * n)(*[r[0] for r in rows]), (C.c_int32 * n)(*[r[1] for r in rows]),
                                        (C.c_double * n)(*[r[2] for r in rows]), (C.c_double * n)(*[r[3] for r in rows]), _p(out[r0:]),
                                        _p(notes[r0:]) if return_notes else None, _p(ws), ws_bytes, _stream()), "harmony_f0_seg")
    return (out, notes) if return_notes else out


def mix_waves(ys, gains, out=None):
    """out[i] = (float)(sum_v gains[v] * (double)ys[v][i]) over 1..4 voices in order (knnsvc_mix_waves; include/knnsvc_hip.h: fp64
    products and sums of their own, one rounding, a voice with gain 0 not read).  ``ys``: contiguous 1-D fp32 tensors of one
    length; ``gains``: linear, finite and >= 0, at least one > 0; ``out``: a buffer to write into, which may be one of ``ys``.
    One launch; enqueue only."""
    ys = list(ys)
    if not 1 <= len(ys) <= HARMONY_MAX_PARTS + 1:
        raise KnnSvcError(f"mix_waves: {len(ys)} voices, expected 1..{HARMONY_MAX_PARTS + 1}")
    for v, y in enumerate(ys):
        _need(y, name=f"ys[{v}]")
        if y.dim() != 1 or not y.is_contiguous() or y.shape != ys[0].shape:
            raise KnnSvcError(f"mix_waves: ys[{v}] must be a contiguous [n] tensor of the voices' common length, got {tuple(y.shape)}")
    gains = [float(g) for g in gains]
    if len(gains) != len(ys):
        raise KnnSvcError(f"mix_waves: {len(gains)} gains for {len(ys)} voices")
    if out is None:
        out = torch.empty_like(ys[0])
    _need(out, name="out")
    if out.shape != ys[0].shape or not out.is_contiguous():
        raise KnnSvcError(f"mix_waves: out must be a contiguous {tuple(ys[0].shape)} tensor, got {tuple(out.shape)}")
    nv = len(ys)
    check(_lib.load().knnsvc_mix_waves((C.c_void_p * nv)(*[y.data_ptr() for y in ys]), nv, (C.c_double * nv)(*gains), ys[0].numel(),
                                       _p(out), _stream()), "mix_waves")
    return out


def weighted_gather(idx4, w, pool, mean=False):
    """sum_k w[i, k] * pool[idx4[i, k]].  ``w`` None = uniform weights: each row times 1.0f / k (softmax(ones)), or with ``mean`` the
    sum in order divided by k (torch.mean); the same bits when k is a power of two."""
    _need(idx4, torch.int64, "idx4")
    idx4 = idx4.contiguous()
    nq, k = idx4.shape
    dim = pool.shape[1]
    out = torch.empty(nq, dim, device=pool.device, dtype=torch.float32)
    check(_lib.load().knnsvc_weighted_gather(_p(idx4), _p(w), nq, k, _p(pool), dim, pool.stride(0), 1 if mean else 0, _p(out),
                                             _stream()), "weighted_gather")
    return out


# ------------------------------------------------------------------ prematch helpers
def round_f16(x):
    """x.half().float() (ddsp_prematch_dataset.py:1509, 1561, 1592) as one pass."""
    _need(x, name="round_f16.x")
    x = x.contiguous()
    out = torch.empty_like(x)
    check(_lib.load().knnsvc_round_f16(_p(x), x.numel(), _p(out), _stream()), "round_f16")
    return out


def amp_ratio(spec_q, spec_pool, idx):
    """[nq,k]: L1(spec_q[t]) / (L1(spec_pool[idx[t,k]]) + 1e-5)  (ddsp_prematch_dataset.py:1657-1660)."""
    _need(spec_q, name="spec_q"); _need(spec_pool, name="spec_pool"); _need(idx, torch.int64, "idx")
    idx = idx.contiguous()
    nq, k = idx.shape
    if spec_q.shape[0] != nq or spec_q.shape[1] != spec_pool.shape[1] or spec_q.stride(1) != 1 or spec_pool.stride(1) != 1:
        raise KnnSvcError("amp_ratio: shape mismatch")
    out = torch.empty(nq, k, device=spec_q.device, dtype=torch.float32)
    check(_lib.load().knnsvc_amp_ratio(_p(spec_q), spec_q.stride(0), _p(spec_pool), spec_pool.stride(0), spec_pool.shape[0],
                                       _p(idx), nq, k, spec_q.shape[1], _p(out), _stream()), "amp_ratio")
    return out


# ------------------------------------------------------------------ f0 front end
def f0_harvest(wav_1d, sample_rate=16000, f0_floor=65.0, f0_ceil=1047.0, frame_period=20.0, zero_below=80.0, check_status=True):
    """Harvest f0 track exactly as the reference asks pyworld for it (ddsp_prematch_dataset.py:121-128):
    [L] fp32 at 16 kHz -> [int(1000 L / fs / frame_period) + 1] fp32, 0 = unvoiced, values below 80 Hz zeroed.  All stages
    on the GPU in fp64 (csrc/harvest.hip); check_status reads the overflow flag back (one host sync)."""
    import ctypes
    _need(wav_1d, name="f0_harvest.wav")
    wav_1d = wav_1d.contiguous()
    lib = _lib.load()
    n, nbytes = ctypes.c_int64(0), ctypes.c_int64(0)
    check(lib.knnsvc_f0_harvest_workspace(wav_1d.numel(), int(sample_rate), float(f0_floor), float(f0_ceil), float(frame_period),
                                          ctypes.byref(n), ctypes.byref(nbytes)), "f0_harvest_workspace")
    ws = torch.empty(nbytes.value, device=wav_1d.device, dtype=torch.uint8)
    out = torch.empty(n.value, device=wav_1d.device, dtype=torch.float32)
    status = torch.zeros(1, device=wav_1d.device, dtype=torch.int32)
    check(lib.knnsvc_f0_harvest(_p(wav_1d), wav_1d.numel(), int(sample_rate), float(f0_floor), float(f0_ceil), float(frame_period),
                                float(zero_below), _p(out), n.value, _p(ws), nbytes.value, _p(status), _stream()), "f0_harvest")
    if check_status:
        flags = int(status.item())
        if flags:
            raise RuntimeError(f"f0_harvest: a fixed-capacity list overflowed (flags {flags:#x}: 1 candidates per frame, "
                               "2 / 4 section storage); the track is incomplete")
    return out


# ------------------------------------------------------------------ side features + synth
def reflect_pad(x1d, pad, extra=0):
    """-> [n + 2 pad (+ extra zeros at the end)]"""
    out = torch.empty(x1d.numel() + 2 * pad + extra, device=x1d.device, dtype=torch.float32)
    if extra:
        out[-extra:].zero_()
    check(_lib.load().knnsvc_reflect_pad(_p(x1d), x1d.numel(), pad, _p(out), _stream()), "reflect_pad")
    return out


def reflect_pad_batch(x_flat, offs, pad, stride):
    """x_flat: signals back to back, offs: device int64 [B+1] -> [B, stride] (reflect-padded rows, zero tails)."""
    B = offs.numel() - 1
    out = torch.empty(B, stride, device=x_flat.device, dtype=torch.float32)
    check(_lib.load().knnsvc_reflect_pad_batch(_p(x_flat), _p(offs), B, pad, _p(out), stride, _stream()), "reflect_pad_batch")
    return out


def spec_harm(reim, bins, f0, n_harm=49):
    """DFT product [rows, 2 bins] + f0 [rows] -> (spec [rows, bins], harm [rows, n_harm]) in one pass."""
    rows = reim.shape[0]
    spec = torch.empty(rows, bins, device=reim.device, dtype=torch.float32)
    harm = torch.empty(rows, n_harm, device=reim.device, dtype=torch.float32)
    check(_lib.load().knnsvc_spec_harm(_p(reim), rows, bins, reim.stride(0), _p(f0), n_harm, _p(spec), _p(harm), _stream()), "spec_harm")
    return spec, harm


def complex_mag(reim, bins):
    rows = reim.shape[0]
    out = torch.empty(rows, bins, device=reim.device, dtype=torch.float32)
    check(_lib.load().knnsvc_complex_mag(_p(reim), rows, bins, reim.stride(0), _p(out), _stream()), "complex_mag")
    return out


def harmonic_amps(spec, f0, n_harm=49):
    T, bins = spec.shape
    out = torch.empty(T, n_harm, device=spec.device, dtype=torch.float32)
    check(_lib.load().knnsvc_harmonic_amps(_p(spec.contiguous()), _p(f0), T, bins, n_harm, _p(out), _stream()),
          "harmonic_amps")
    return out


def additive_synth(f0, amp, prenet_w, prenet_b, cond, ld_cond, *, hop=320, sr=16000, mode=0, want_exc=False, n_dyn=None):
    """f0 [N], amp [N,H] (None in sine mode) -> writes cond (a [N*hop, >=n_ch] view); returns exc or None."""
    N = f0.numel()
    n_ch = prenet_b.numel()
    H = amp.shape[1] if amp is not None else 0
    exc = torch.empty(N * hop, device=f0.device, dtype=torch.float32) if want_exc else None
    ph = torch.empty(N, device=f0.device, dtype=torch.float64)
    check(_lib.load().knnsvc_additive_synth(_p(f0), _p(amp), N, H, hop, sr, mode, _p(prenet_w), _p(prenet_b), n_ch,
                                            _p(cond), ld_cond, _p(exc), _p(ph), _p(n_dyn), _stream()), "additive_synth")
    return exc


# ------------------------------------------------------------------ output loudness
def loudness_layout():
    """(samples one lane filters, samples one workgroup covers) as the library reports them (csrc/loudness.hip: LD_C, LD_W): the
    lengths at which the measure changes path; the filter state crosses the first kind of boundary."""
    chunk, group = C.c_int32(0), C.c_int32(0)
    _lib.load().knnsvc_loudness_layout(C.byref(chunk), C.byref(group))
    return chunk.value, group.value


def loudness(wav, sample_rate=16000, return_counts=False):
    """Integrated loudness (LKFS) of a mono signal after ITU-R BS.1770-4 — K-weighting, 400 ms blocks, absolute gate at -70 and
    relative gate at -10 (the definition in include/knnsvc_hip.h; fp64 on the device, csrc/loudness.hip) -> 0-d fp32 device
    tensor, -inf for a signal shorter than one block or one that the gates empty.  return_counts: (lkfs, int32 [3] = blocks,
    blocks kept by the absolute gate, blocks kept by both).  Enqueue only: no host read."""
    _need(wav, name="loudness.wav")
    if wav.dim() != 1:
        raise KnnSvcError(f"loudness: expected a mono waveform [L], got shape {tuple(wav.shape)}")
    wav = wav.contiguous()
    lib = _lib.load()
    n = wav.numel()
    nbytes = lib.knnsvc_loudness_workspace_bytes(n, int(sample_rate))
    if nbytes == 0:
        check(1, "loudness_workspace_bytes")
    ws = torch.empty((nbytes + 7) // 8, device=wav.device, dtype=torch.float64)
    lkfs = torch.empty((), device=wav.device, dtype=torch.float32)
    counts = torch.empty(3, device=wav.device, dtype=torch.int32) if return_counts else None
    check(lib.knnsvc_loudness(_p(wav), n, int(sample_rate), _p(lkfs), _p(counts), _p(ws), ws.numel() * 8, _stream()), "loudness")
    return (lkfs, counts) if return_counts else lkfs


def normalize_loudness(wav, target_db, sample_rate=16000, out=None):
    """wav scaled to ``target_db`` LKFS: out = wav * 10^((target_db - loudness(wav)) / 20) -> (out, lkfs of wav as a 0-d device
    tensor).  A signal without a measurable loudness (-inf: silence, or shorter than 400 ms) comes back unchanged.  ``out`` may
    be ``wav`` itself (in place).  Enqueue only: no host read.  This op does not limit the result: a quiet, peaky signal can pass
    full scale, and audio_io.save_audio then divides by the peak (the reference's rule), so the FILE is lower than asked —
    unless ``limit_peak`` (below; the ``peak_db`` switch of the entry points) holds the peaks under a ceiling first, at the
    price of a loudness that can end below ``target_db`` where the limiter engages."""
    _need(wav, name="normalize_loudness.wav")
    if not wav.is_contiguous():
        raise KnnSvcError("normalize_loudness: expected a contiguous waveform")
    lkfs = loudness(wav, sample_rate)
    if out is None:
        out = torch.empty_like(wav)
    elif not (_need(out, name="normalize_loudness.out").is_contiguous() and out.shape == wav.shape):
        raise KnnSvcError("normalize_loudness: out must be a contiguous fp32 tensor of wav's shape")
    check(_lib.load().knnsvc_loudness_gain(_p(wav), wav.numel(), _p(lkfs), float(target_db), _p(out), _stream()), "loudness_gain")
    return out, lkfs


# ------------------------------------------------------------------ output dynamics
def _dyn_out(name, y, out):
    _need(y, name=f"{name}.y")
    if y.dim() != 1 or not y.is_contiguous():
        raise KnnSvcError(f"{name}: expected a contiguous mono waveform [L], got shape {tuple(y.shape)}")
    if out is None:
        return torch.empty_like(y)
    if not (_need(out, name=f"{name}.out").is_contiguous() and out.shape == y.shape):
        raise KnnSvcError(f"{name}: out must be a contiguous fp32 tensor of y's shape")
    return out


def envelope_mix(y, x, a, hop=320, out=None, return_gains=False):
    """The shape of the source's volume envelope put back on a generated waveform: ``y`` [T hop] scaled frame by frame by
    G[t] = min((px[t] / py[t])^a, 4), px / py the three-block RMS envelopes of the source ``x`` (zero-extended or cut to y's
    length) and of y, each relative to its own global RMS and floored at 1e-3, G interpolated linearly between frame centres
    (the definition in include/knnsvc_hip.h; fp64 on the device, csrc/dynamics.hip).  ``a`` in [0, 1]: 0 leaves y as it is, 1
    transfers the envelope fully.  Level-invariant: scaling x changes nothing.  A silent x or y gives y back bit for bit.
    -> out, or (out, G as [T] fp64 device tensor) with return_gains.  ``out`` may be ``y`` itself.  Enqueue only: no host read."""
    out = _dyn_out("envelope_mix", y, out)
    _need(x, name="envelope_mix.x")
    if x.dim() != 1:
        raise KnnSvcError(f"envelope_mix: expected a mono source waveform [L], got shape {tuple(x.shape)}")
    x = x.contiguous()
    lib = _lib.load()
    n = y.numel()
    nbytes = lib.knnsvc_envelope_workspace_bytes(n, int(hop))
    if nbytes == 0:
        check(1, "envelope_workspace_bytes")
    ws = torch.empty((nbytes + 7) // 8, device=y.device, dtype=torch.float64)
    gains = torch.empty(n // int(hop), device=y.device, dtype=torch.float64) if return_gains else None
    check(lib.knnsvc_envelope_mix(_p(y), n, _p(x), x.numel(), int(hop), float(a), _p(out), _p(gains), _p(ws), ws.numel() * 8,
                                  _stream()), "envelope_mix")
    return (out, gains) if return_gains else out


def peak_limit_layout():
    """(samples per workgroup tile, look-ahead L at 16 kHz) as the library reports them (csrc/dynamics.hip: PK_TILE, and
    L = floor(0.005 sample_rate + 0.5)): the lengths and positions at which ``limit_peak`` changes path."""
    tile, look = C.c_int32(0), C.c_int32(0)
    _lib.load().knnsvc_peak_limit_layout(C.byref(tile), C.byref(look))
    return tile.value, look.value


def limit_peak(y, peak_db, sample_rate=16000, out=None, return_stats=False):
    """A sample-peak ceiling at ``peak_db`` dBFS (<= 0): a look-ahead limiter without recursion — the gain each sample needs, its
    minimum over +-5 ms, smoothed by a 10 ms Hann (the definition in include/knnsvc_hip.h; fp64 on the device,
    csrc/dynamics.hip).  |out| <= 10^(peak_db / 20) (1 + 2^-23) everywhere; samples further than 10 ms from anything over the
    ceiling come back bit-identical.  Not a true-peak limiter, and it does not bring the loudness back.
    -> out, or (out, (int64 0-d device tensor: samples whose gain is below 1, fp64 0-d device tensor: the smallest gain)) with
    return_stats.  ``out`` may be ``y`` itself (one workgroup then walks the signal in order: same bits, slower).  Enqueue
    only: no host read."""
    out = _dyn_out("limit_peak", y, out)
    stats = torch.empty(2, device=y.device, dtype=torch.int64) if return_stats else None
    check(_lib.load().knnsvc_peak_limit(_p(y), y.numel(), int(sample_rate), float(peak_db), _p(out), _p(stats), _stream()), "peak_limit")
    return (out, (stats[0], stats[1:].view(torch.float64)[0])) if return_stats else out


# ------------------------------------------------------------------ pool-silence trimming
def vad_trim(wavs, trigger_level, sample_rate=16000, return_measures=False):
    """Where speech starts and ends in every recording of ``wavs`` (a list of mono fp32 device tensors [L_i], or one such tensor):
    the sox `vad` effect with torchaudio's default parameters applied to both ends, every cut a whole number of 320-sample hops,
    as restated in include/knnsvc_hip.h (fp64 on the device, csrc/vad.hip; that restatement, mirrored by tests/vad_oracle.py, is
    the specification — parity with torchaudio's own code is not pinned) -> int64 device tensor [n, 2] = (lstrip, rstrip): keep
    wav[lstrip : L - rstrip]; (-1, -1) for a recording to drop (no speech found from one of its ends, or less than one
    measurement left).  return_measures: (strip, [(forward, reversed) fp64 device vectors of each recording's measures]).
    Enqueue only: no host read.  A recording's result does not depend on the others in the call."""
    one = isinstance(wavs, torch.Tensor)
    wavs = [wavs] if one else list(wavs)
    if not wavs:
        raise KnnSvcError("vad_trim: no recording")
    for w in wavs:
        _need(w, name="vad_trim.wav")
        if w.dim() != 1 or w.numel() == 0:
            raise KnnSvcError(f"vad_trim: expected non-empty mono waveforms [L], got shape {tuple(w.shape)}")
    level = float(trigger_level)
    if not (math.isfinite(level) and level > 0.0):
        raise KnnSvcError(f"vad_trim: trigger_level must be finite and positive, got {trigger_level!r}")
    lib = _lib.load()
    dev = wavs[0].device
    x = wavs[0].contiguous() if len(wavs) == 1 else torch.cat([w.contiguous() for w in wavs])
    strip = torch.empty(len(wavs), 2, device=dev, dtype=torch.int64)
    measures = []
    for a, r0, tab in Segments.of_lengths(w.numel() for w in wavs).chunks:
        n, total = len(tab) - 1, int(tab[len(tab) - 1])
        nbytes = lib.knnsvc_vad_workspace_bytes(total, n, int(sample_rate))
        if nbytes == 0:
            check(1, "vad_workspace_bytes")
        ws = torch.empty((nbytes + 7) // 8, device=dev, dtype=torch.float64)
        period = int(sample_rate / 20.0 + .5)
        rows = total // period + 1
        meas = torch.empty(2, rows, device=dev, dtype=torch.float64) if return_measures else None
        check(lib.knnsvc_vad_trim_seg(_p(x[r0:]), tab, n, int(sample_rate), level, _p(strip[a:]), _p(meas), _p(ws), ws.numel() * 8,
                                      _stream()), "vad_trim_seg")
        if return_measures:
            mlen = int(sample_rate * 0.1 + .5)
            for s in range(n):
                L, at = int(tab[s + 1] - tab[s]), int(tab[s]) // period
                M = (L - mlen) // period + 1 if L >= mlen else 0
                measures.append((meas[0, at:at + M], meas[1, at:at + M]))
    return (strip, measures) if return_measures else strip
