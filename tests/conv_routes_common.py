"""The route table of knnsvc_conv_gemm: one row per kernel tag the dispatcher (knn_svc_amd/csrc/conv_gemm.hip) can report through
ops.last_conv_kernel(), with the descriptor that reaches it, plus the yardsticks every row is held to: the same operation in fp64
(F.conv1d / F.conv_transpose1d and the epilogue chain in the kernel's order) and in fp32, both with torch on the CPU.

Imports without a GPU.  tests/test_conv_routes_cpu.py checks the table against what the dispatcher itself answers (`route`: the
row's descriptors handed to ops.conv_route, which launches nothing); tests/conv_routes_child.py launches every row,
tests/test_gpu_conv_routes.py judges what it measured.

Shapes are ragged on purpose: m is a whole number of tiles plus an odd remainder (or less than one tile), n is no multiple of the
tile width, every output has `COL_SLACK` columns behind n and `ROW_GAP` rows around every batch item that no launch may touch."""
from __future__ import annotations

import functools
import os
from dataclasses import dataclass, replace

import torch
import torch.nn.functional as F

ACT_NONE, ACT_GELU, ACT_LRELU, ACT_TANH = 0, 1, 2, 3
ROW_GAP = 4          # sentinel rows in front of the first and behind every batch item (o_bstride = (rows + ROW_GAP) * ldo)
COL_SLACK = 4        # sentinel columns n .. ldo (a multiple of 4: the 16-byte epilogue stays reachable)
SENTINEL = -12345.678


@dataclass(frozen=True)
class Case:
    id: str
    tag: str                    # what ops.last_conv_kernel() must say
    m: int                      # GEMM rows per batch item (transposed: t + taps - 1)
    n: int                      # GEMM columns per group (transposed: u * cout)
    k: int = 1                  # taps of the GEMM (transposed: kernel / u)
    cin: int = 32
    stride: int = 1
    dil: int = 1
    pad: int = -1               # -1: (k - 1) * dil / 2 at stride 1, k / 2 otherwise
    t_in: int = -1              # -1: the longest input that gives m rows
    batches: int = 1
    groups: int = 1
    split: str = "f16x2"        # KNNSVC_GEMM at attach_split time; "" = unsplit weights (fp32 MFMA)
    x_split: bool = False       # input handed over in the f16x2 split layout
    a_slope: float = 1.0
    bias: bool = True
    act: int = ACT_NONE
    act_slope: float = 0.1
    resid: bool = False
    ldr_extra: int = 0          # ldr = width + ldr_extra (ldo = width + COL_SLACK: never equal unless asked)
    accumulate: bool = False
    div: float = 1.0
    convt: tuple = ()           # (u, cout): transposed convolution of stride u, kernel k * u, padding (k * u - u) / 2
    slot: bool = False          # pass out_absmax
    epi: str | None = None      # what ops.last_conv_epilogue() must say (None: not checked)
    env: tuple = ()             # dispatcher knobs ((name, value), ...) this row may set
    branches: tuple = ()        # multi-descriptor rows: ((k, dil), ...), one descriptor each over the same input
    seed: int = 0

    @property
    def family(self) -> str:
        return {"G": "fp32", "H": "bf16x3"}.get(self.tag[0], "f16x2")

    @property
    def pad_(self) -> int:
        if self.convt:
            return 0
        if self.pad >= 0:
            return self.pad
        return (self.k - 1) * self.dil // 2 if self.stride == 1 else self.k // 2

    @property
    def t_in_(self) -> int:
        if self.convt:
            return self.m - self.k + 1
        if self.t_in >= 0:
            return self.t_in
        return (self.m - 1) * self.stride + self.dil * (self.k - 1) + 1 - 2 * self.pad_ + (self.stride - 1)

    @property
    def width(self) -> int:      # valid output columns of a row
        return self.convt[1] if self.convt else self.groups * self.n

    @property
    def rows(self) -> int:       # valid output rows of a batch item
        return self.t_in_ * self.convt[0] if self.convt else self.m

    @property
    def ldo(self) -> int:
        return self.width + COL_SLACK

    @property
    def ldr(self) -> int:
        return self.width + self.ldr_extra

    def descs(self):
        """The single-descriptor cases this row launches: itself, or one per branch."""
        if not self.branches:
            return [self]
        return [replace(self, k=k, dil=d, branches=(), seed=self.seed + 1000 * (i + 1)) for i, (k, d) in enumerate(self.branches)]


def _c(id, tag, m, n, **kw):
    return Case(id=id, tag=tag, m=m, n=n, **kw)


LRELU = dict(act=ACT_LRELU, a_slope=0.1)          # the generator's first convolution of a ResBlock pair: lane epilogue
_WIN = dict(slot=True, epi="patch")
_B3 = ((11, 3), (7, 3), (3, 3))                   # the generator's three branches
_B4 = ((11, 3), (7, 5), (5, 1), (3, 3))

CASES = [
    # ---- windowed kernels, by the tile-shape rules (default knobs)
    _c("W128D", "W128D", 333, 72, k=3, batches=2, **_WIN),
    _c("W128S", "W128S", 2501, 100, k=7, dil=3, batches=8, a_slope=0.1, resid=True, **_WIN),
    _c("W128", "W128", 261, 72, k=3, batches=171, **_WIN),
    _c("W160", "W160", 641, 72, k=3, batches=140, a_slope=0.1, **_WIN),
    _c("W64", "W64", 517, 40, k=11, dil=5, **_WIN),
    _c("W32", "W32", 517, 20, k=7, batches=3, **_WIN),
    _c("W64P", "W64P", 301, 64, k=11, dil=10, **_WIN),
    # WavLM's positional convolution: 1024 channels in 16 groups, k = 128 (even: one more row of padding in front), GELU + residual
    _c("W64P-grouped", "W64P", 45, 64, k=128, cin=64, pad=64, t_in=45, batches=2, groups=16, act=ACT_GELU, resid=True, slot=True, epi="lane"),
    # ---- tap-major f16x2 kernels
    _c("F64S", "F64S", 199, 96, k=3, stride=2, slot=True, epi="patch"),
    _c("F128", "F128", 2101, 130, k=3, stride=2, batches=8, a_slope=0.1, slot=True, epi="lane"),
    _c("F64", "F64", 301, 40, k=4, stride=2, slot=True, epi="patch"),
    _c("F32", "F32", 301, 20, k=16, stride=8, act=ACT_TANH, slot=True, epi="lane"),
    # ---- several descriptors in one grid (conv_gemm(..., defer=) + conv_gemm_multi)
    _c("W128Dx", "W128Dx", 777, 128, branches=_B3, slot=True, **LRELU),
    _c("W128Sx", "W128Sx", 6001, 128, branches=_B3, slot=True, resid=True),
    _c("W128x", "W128x", 16500, 72, branches=_B4, slot=True),
    _c("W160x", "W160x", 30001, 72, branches=_B4, slot=True, **LRELU),
    _c("W64x", "W64x", 517, 40, branches=_B3, slot=True, act=ACT_TANH),
    _c("W32x", "W32x", 301, 20, branches=_B3, slot=True, resid=True),
    _c("W64Px", "W64Px", 301, 50, branches=((11, 10), (9, 10), (7, 12)), slot=True),
    # ---- pre-split input (the encoder's layout); the quad kernel by shape
    _c("F128a2", "F128a2", 2101, 130, k=3, stride=2, batches=8, x_split=True, slot=True, epi="lane"),
    _c("F64-a2", "F64", 301, 40, k=4, stride=2, x_split=True, slot=True, epi="patch"),
    _c("F32-a2", "F32", 301, 20, cin=96, x_split=True, act=ACT_GELU, slot=True, epi="lane"),
    _c("Q256S", "Q256S", 31, 260, cin=1024, x_split=True, epi=""),
    _c("Q256S-gelu", "Q256S", 31, 260, cin=1024, x_split=True, act=ACT_GELU, epi=""),
    _c("Q256S-resid-slot", "Q256S", 31, 260, cin=1024, x_split=True, resid=True, slot=True, epi=""),
    # ---- bf16x3
    _c("H128", "H128", 301, 130, k=3, batches=2, split="bf16x3", a_slope=0.1, resid=True, epi=""),
    _c("H64", "H64", 301, 40, k=4, stride=2, split="bf16x3", act=ACT_GELU, epi=""),
    _c("H32", "H32", 517, 20, k=7, dil=3, batches=3, split="bf16x3", accumulate=True, div=3.0, epi=""),
    # ---- fp32 MFMA: unsplit weights; v8 = cin % 32 == 0, v4 = cin % 4 == 0, v1 = anything
    _c("G128v8", "G128v8", 301, 130, k=3, batches=2, split="", a_slope=0.1, resid=True, epi=""),
    _c("G64v8", "G64v8", 301, 40, k=4, stride=2, split="", act=ACT_GELU, epi=""),
    _c("G32v8", "G32v8", 517, 20, k=7, dil=3, batches=3, split="", accumulate=True, div=3.0, epi=""),
    _c("G128v4", "G128v4", 301, 130, k=3, cin=36, batches=2, split="", act=ACT_LRELU, epi=""),
    _c("G64v4", "G64v4", 301, 40, k=4, cin=36, stride=2, split="", resid=True, epi=""),
    _c("G32v4", "G32v4", 517, 20, k=7, cin=36, dil=3, split="", act=ACT_TANH, epi=""),
    _c("G128v1-cin34", "G128v1", 301, 130, k=3, cin=34, batches=2, split="", a_slope=0.1, epi=""),
    _c("G64v1-cin1", "G64v1", 301, 40, k=10, cin=1, stride=5, split="", act=ACT_GELU, epi=""),
    _c("G32v1-cin34", "G32v1", 301, 20, k=16, cin=34, stride=8, split="", resid=True, epi=""),
    _c("G128v1-cin1", "G128v1", 301, 130, k=10, cin=1, stride=5, split="", epi=""),
    _c("G64v1-cin34", "G64v1", 301, 40, k=7, cin=34, dil=3, batches=2, split="", epi=""),
    _c("G32v1-cin1", "G32v1", 517, 20, k=7, cin=1, split="", accumulate=True, div=2.0, epi=""),
    # ---- transposed convolutions (the generator's upsamplers): one per tap-major tile, patch epilogue
    _c("F128-convt", "F128", 4101, 128, k=2, dil=-1, batches=8, convt=(8, 16), a_slope=0.1, slot=True, epi="patch"),
    _c("F64S-convt", "F64S", 58, 128, k=2, dil=-1, convt=(8, 16), a_slope=0.1, slot=True, epi="patch"),
    _c("F64-convt", "F64", 302, 40, k=2, dil=-1, convt=(2, 20), a_slope=0.1, slot=True, epi="patch"),
    _c("F32-convt", "F32", 303, 16, k=3, dil=-1, convt=(2, 8), a_slope=0.1, slot=True, epi="patch"),
    # ---- knobs
    _c("W128D-generic-epilogue", "W128D", 333, 72, k=3, batches=2, resid=True, slot=True, epi="lane", env=(("KNNSVC_EPILOGUE", "g"),)),
    _c("F64-win-off", "F64", 517, 40, k=11, dil=5, batches=2, slot=True, epi="patch", env=(("KNNSVC_WIN", "0"),)),
    # ---- edges
    _c("W128D-one-row", "W128D", 1, 72, k=3, **_WIN),
    _c("W64-shorter-than-halo", "W64", 7, 40, k=11, dil=5, **_WIN),
    _c("W128D-resid-other-pitch", "W128D", 333, 72, k=3, batches=2, resid=True, ldr_extra=12, **_WIN),
]
CASES = [replace(c, seed=100 + i) for i, c in enumerate(CASES)]
BY_ID = {c.id: c for c in CASES}
assert len(BY_ID) == len(CASES)

# bucketed launches (dyn = (count, bucket)): (row at the bucket's size, rows per count, count, bucket); batches == 1
DYN_CASES = [
    (_c("W128D-dyn", "W128D", 42 * 8, 72, k=3, resid=True, **_WIN), 8, 39, 42),
    (_c("W128S-dyn", "W128S", 2500 * 8, 100, k=7, dil=3, a_slope=0.1, **_WIN), 8, 2497, 2500),
    (_c("W64-dyn", "W64", 70 * 8, 40, k=11, dil=5, **_WIN), 8, 65, 70),
    (_c("W32-dyn", "W32", 70 * 8, 20, k=7, **_WIN), 8, 33, 70),
    (_c("F64S-convt-dyn", "F64S", 61, 128, k=2, dil=-1, convt=(8, 16), a_slope=0.1, slot=True, epi="patch"), 1, 53, 60),
]
DYN_CASES = [(replace(c, seed=900 + i), f, cnt, nb) for i, (c, f, cnt, nb) in enumerate(DYN_CASES)]


def dyn_exact(case: Case, per: int, count: int, bucket: int) -> Case:
    """The exact-length row of a bucketed one: every length at `count` instead of `bucket`."""
    return replace(case, m=case.m - (bucket - count) * per)


# ------------------------------------------------------------------ inputs and references
def make_inputs(case: Case) -> dict:
    """Seeded host tensors of one single-descriptor case: x [B, t_in, G * cin], the weight in torch's layout, bias, residual and the
    previous output content (accumulate).  A pre-split input is rounded to what the split layout holds, which is what the kernel
    is given."""
    assert not case.branches
    g = torch.Generator().manual_seed(case.seed)
    B, G = case.batches, case.groups
    x = torch.randn(B, case.t_in_, G * case.cin, generator=g)
    if case.x_split:
        from knn_svc_amd import ops
        x = ops.split_unpack(ops.split_pack(x.view(-1, G * case.cin))).view_as(x).contiguous()
    if case.convt:
        u, cout = case.convt
        w = torch.randn(case.cin, cout, case.k * u, generator=g) / (case.cin * case.k) ** 0.5
    else:
        w = torch.randn(G * case.n, case.cin, case.k, generator=g) / (case.cin * case.k) ** 0.5
    inp = dict(x=x, w=w)
    inp["bias"] = torch.randn(case.width, generator=g) if case.bias else None
    inp["resid"] = torch.randn(B, case.rows, case.width, generator=g) if case.resid else None
    inp["prev"] = torch.randn(B, case.rows, case.width, generator=g) if case.accumulate else None
    return inp


def reference(case: Case, inp: dict, dtype) -> torch.Tensor:
    """[B, rows, width]: the descriptor's operation with torch on the CPU in `dtype`, epilogue in the kernel's order:
    input leaky ReLU, convolution, bias, activation, residual, accumulate, divide."""
    cvt = lambda t: None if t is None else t.to(dtype)
    x = cvt(inp["x"]).transpose(1, 2)
    if case.a_slope != 1.0:
        x = F.leaky_relu(x, case.a_slope)
    if case.convt:
        u = case.convt[0]
        v = F.conv_transpose1d(x, cvt(inp["w"]), None, stride=u, padding=(case.k * u - u) // 2)
    else:
        need = (case.m - 1) * case.stride + case.dil * (case.k - 1) + 1           # padded input rows that m outputs consume
        x = F.pad(x, (case.pad_, need - case.pad_ - case.t_in_))
        v = F.conv1d(x, cvt(inp["w"]), None, stride=case.stride, dilation=case.dil, groups=case.groups)
    v = v.transpose(1, 2)
    assert v.shape == (case.batches, case.rows, case.width), (v.shape, case)
    if inp["bias"] is not None:
        v = v + cvt(inp["bias"])
    if case.act == ACT_GELU:
        v = F.gelu(v)
    elif case.act == ACT_LRELU:
        v = F.leaky_relu(v, case.act_slope)
    elif case.act == ACT_TANH:
        v = torch.tanh(v)
    if inp["resid"] is not None:
        v = v + cvt(inp["resid"])
    if inp["prev"] is not None:
        v = v + cvt(inp["prev"])
    if case.div != 1.0:
        v = v / case.div
    return v.contiguous()


@functools.lru_cache(maxsize=None)
def prepared(case: Case):
    """-> (inputs, ref64, e32, scale) of a single-descriptor case, computed once and shared; nobody writes to them.
    e32 = max |fp32 on the CPU - fp64|: the unit every route's error is measured in."""
    inp = make_inputs(case)
    ref64 = reference(case, inp, torch.float64)
    e32 = float((reference(case, inp, torch.float32).double() - ref64).abs().max())
    return inp, ref64, e32, float(ref64.abs().max())


def tolerance(factor: float, e32: float, scale: float) -> float:
    return factor * e32 + 1e-6 * scale


# ------------------------------------------------------------------ a row's descriptors, and what the dispatcher says to them
def _ops():
    from knn_svc_amd import ops
    return ops


class Knobs:
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


class Launch:
    """One descriptor of a row on `dev`: operands, the sentinel-framed output buffer and the conv_gemm call.  On "cpu" nothing can
    be launched, but `launch(defer=descs)` builds the same descriptor (ops.conv_route takes it): attach_split needs a GPU, so a
    few zero bytes stand in for the split planes there — the dispatcher looks at their address, never behind it."""

    def __init__(self, case, inp, rows_alloc=None, x_rows_alloc=None, dev="cuda"):
        ops = _ops()
        self.case, c = case, case
        B, G = c.batches, c.groups
        self.rows_alloc = rows_alloc or c.rows                      # a bucketed launch is laid out for more rows than are valid
        x = inp["x"]
        if x_rows_alloc:                                            # rows behind the valid input: finite junk the kernel must not read
            x = torch.cat([x, torch.full((B, x_rows_alloc - x.shape[1], x.shape[2]), 7.0)], 1)
        self.t_alloc = x.shape[1]
        x2d = x.reshape(-1, G * c.cin)
        self.x = (ops.split_pack(x2d) if c.x_split else x2d.contiguous()).to(dev)
        if c.convt:
            wp = ops.pack_convT_weight(inp["w"], c.convt[0])
        elif G > 1:
            wp = ops.pack_grouped_conv_weight(inp["w"], G)
        else:
            wp = ops.pack_conv_weight(inp["w"])
        self.w = wp.to(dev)
        if c.split and dev == "cpu":
            planes = torch.zeros(8, dtype=torch.int16)
            if c.split == "bf16x3":
                self.w._w3 = planes
            else:
                self.w._w2, self.w._w2_scale = planes, 1.0
        elif c.split:
            self.w = ops.attach_split(self.w)
            assert hasattr(self.w, "_w3" if c.split == "bf16x3" else "_w2"), "the weights did not take the split this row is about"
        self.bias = inp["bias"].to(dev) if inp["bias"] is not None else None
        self.resid = None
        if inp["resid"] is not None:
            r = torch.zeros(B, c.rows, c.ldr)
            r[:, :, :c.width] = inp["resid"]
            self.resid = r.to(dev)
        self.prev = inp["prev"]
        self.pitch = self.rows_alloc + ROW_GAP                      # rows from one batch item's block to the next
        self.buf = torch.empty(ROW_GAP + B * self.pitch, c.ldo, device=dev)
        self.slot = ops.new_slot(dev) if c.slot else None
        self.reset()

    def reset(self):
        c = self.case
        self.buf.fill_(SENTINEL)
        if self.prev is not None:
            self._blocks()[:, :c.rows, :c.width] = self.prev.to(self.buf.device)
        if self.slot is not None:
            self.slot.zero_()

    def _blocks(self):
        return self.buf[ROW_GAP:].view(self.case.batches, self.pitch, self.case.ldo)

    def valid(self, rows=None):
        return self._blocks()[:, :rows or self.case.rows, :self.case.width]

    def outside_is_untouched(self, rows=None):
        """Every float outside the [rows, width] blocks still holds the sentinel's bits."""
        mask = torch.ones_like(self.buf, dtype=torch.bool)
        mask[ROW_GAP:].view(self.case.batches, self.pitch, self.case.ldo)[:, :rows or self.case.rows, :self.case.width] = False
        return bool((self.buf[mask] == SENTINEL).all()), int((self.buf[mask] != SENTINEL).sum())

    def launch(self, defer=None, dyn=None, m_alloc=None):
        """conv_gemm of this descriptor (defer: appended to the list instead).  dyn = (count, bucket) with m_alloc: this
        (exact-length) descriptor's data through a launch laid out for the bucket's m_alloc rows."""
        ops, c = _ops(), self.case
        B, G = c.batches, c.groups
        ldx = G * c.cin
        kw = dict(m=c.m if dyn is None else m_alloc, n=c.n, cin=c.cin, taps=c.k, stride=c.stride, dil=c.dil, pad=c.pad_,
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
        ops.conv_gemm(self.x, self.w, self.buf[ROW_GAP:], **kw)

    def route(self, **kw):
        """What the dispatcher says to this descriptor alone, without a launch."""
        descs = []
        self.launch(defer=descs, **kw)
        return _ops().conv_route(descs)


def route(case: Case) -> tuple:
    """-> (tag, epilogue) the library picks for this row under the row's knobs, asked on the CPU: the descriptors are the ones
    the GPU child launches (Launch), one per branch for a merged grid."""
    with Knobs(case):
        descs = []
        for d in case.descs():
            Launch(d, make_inputs(d), dev="cpu").launch(defer=descs)
        return _ops().conv_route(descs)
