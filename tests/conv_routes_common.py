"""The route table of knnsvc_conv_gemm: one row per kernel tag the dispatcher (knn_svc_amd/csrc/conv_gemm.hip) can report through
ops.last_conv_kernel(), with the descriptor that reaches it, plus the yardsticks every row is held to: the same operation in fp64
(F.conv1d / F.conv_transpose1d and the epilogue chain in the kernel's order) and in fp32, both with torch on the CPU.

Imports without a GPU.  tests/test_conv_routes_cpu.py checks the table against the dispatcher's source and against `predict`, a
host mirror of the dispatch rules; tests/conv_routes_child.py launches every row, tests/test_gpu_conv_routes.py judges what it measured.

Shapes are ragged on purpose: m is a whole number of tiles plus an odd remainder (or less than one tile), n is no multiple of the
tile width, every output has `COL_SLACK` columns behind n and `ROW_GAP` rows around every batch item that no launch may touch."""
from __future__ import annotations

import functools
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


# ------------------------------------------------------------------ host mirror of the dispatch rules (conv_gemm.hip)
def _cdiv(a, b):
    return -(-a // b)


def _win_shape(c: Case, z: int, knobs: dict) -> str | None:
    if c.x_split or c.convt or c.stride != 1 or c.k < 3 or c.dil < 1 or (c.groups * c.cin) % 4 or knobs.get("KNNSVC_WIN") == "0":
        return None
    halo = (c.k - 1) * c.dil
    if halo <= 64:
        if c.n > 64:
            if _cdiv(c.m, 128) * _cdiv(c.n, 128) * z < 512:
                return "W128D" if _cdiv(c.m, 64) * _cdiv(c.n, 128) * z <= 256 else "W128S"
            zz = z * _cdiv(c.n, 128)
            r128 = _cdiv(_cdiv(c.m, 128) * zz, 768) * 128
            r160 = _cdiv(_cdiv(c.m, 160) * zz, 768) * 160
            return "W160" if r160 < r128 else "W128"
        return "W64" if c.n > 32 else "W32"
    if halo <= 128 and 32 < c.n <= 64:
        return "W64P"
    return None


def wide_ok(c: Case, knobs: dict) -> bool:
    """The preconditions of the 16-byte LDS-patch epilogue that depend on the descriptor (the buffers here are 16-byte aligned)."""
    generic = knobs.get("KNNSVC_EPILOGUE") == "g"
    lin = not c.convt and not generic
    plain_t = bool(c.convt) and not c.resid and c.convt[1] % 4 == 0
    n, ldo = c.n, c.ldo
    return ((lin or plain_t) and c.act == ACT_NONE and not c.accumulate and c.div == 1.0 and n % 4 == 0 and ldo % 4 == 0 and
            (not c.resid or c.ldr % 4 == 0) and (not c.bias or (c.convt[1] if c.convt else 0) % 4 == 0) and
            (c.groups == 1 or n % 4 == 0))


def predict(case: Case) -> tuple:
    """-> (tag, epilogue) the dispatcher picks for this row under the row's knobs (epilogue None for a merged grid: the hook
    reports single launches)."""
    knobs = dict(case.env)
    ds = case.descs()
    c = ds[0]
    ldx = c.groups * c.cin
    vec4 = c.cin % 4 == 0 and ldx % 4 == 0
    fast = vec4 and c.cin % 32 == 0
    if fast and c.split == "f16x2":
        K = c.cin * c.k
        quad_ok = c.x_split and not c.convt and knobs.get("KNNSVC_EPILOGUE") != "g" and c.n % 4 == 0 and c.ldo % 4 == 0 and (not c.resid or c.ldr % 4 == 0)
        if quad_ok and c.n >= 256 and K >= 1024:
            return "Q256S", ""
        epi = "patch" if wide_ok(c, knobs) else "lane"
        if len(ds) > 1:
            shapes = {_win_shape(d, len(ds), knobs) for d in ds}
            assert len(shapes) == 1 and None not in shapes and c.batches == 1 and c.groups == 1, (case.id, shapes)
            return shapes.pop() + "x", None
        ws = _win_shape(c, c.batches * c.groups, knobs)
        if ws:
            return ws, epi
        if c.n > 64 and _cdiv(c.m, 128) * _cdiv(c.n, 128) * c.batches * c.groups < 256:
            return "F64S", epi
        return ("F128a2" if c.x_split else "F128") if c.n > 64 else "F64" if c.n > 32 else "F32", epi
    assert len(ds) == 1 and not c.x_split
    size = "128" if c.n > 64 else "64" if c.n > 32 else "32"
    if fast and c.split == "bf16x3":
        return "H" + size, ""
    return "G" + size + ("v8" if fast else "v4" if vec4 else "v1"), ""
