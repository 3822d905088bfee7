"""The route table of knnsvc_wavlm_attention: one row per shape, input family and flag combination with the kernel tag the
dispatcher (knn_svc_amd/csrc/attention.hip) must report through ops.last_attention_kernel(), plus the yardstick every row is held
to: `attention_ref`, a plain evaluation with an explicit score matrix and an ordinary softmax, in float64 (the reference) and in
float32 (e32, what an fp32 evaluation of the same inputs loses), both with torch on the CPU.

Imports without a GPU.  `route`, `longest_T` and `schedules` are what the dispatcher itself answers through its host-only route
entry, which launches nothing.  tests/test_attention_cpu.py checks the reference against torch's SDPA and the oracle's bias path,
the table against `route` at every row and at the dispatch rules' boundaries, and that every input family reaches the branch it
is named for.  tests/attention_child.py / attention_fp32_child.py launch the rows,
tests/test_gpu_attention.py judges what they measured.

Layout of the operands (as the kernels read them): q, k, v [B, T, H, 64], gate [B, T, H], table [H, 2T - 1];
score[b, h, i, j] = q . k / 8 + gate[b, i, h] * table[h, j - i + T - 1]; batch row b attends to keys j < clamp(kv_len[b], 1, T)."""
from __future__ import annotations

import functools
import os
from dataclasses import dataclass

import torch

HD = 64
A2_LIMIT = 0.9 * 65504.0 / 16.0        # WavLMEncoder.A2_LIMIT: |k|, |v| the f16x2 route admits (|q| up to 5 x that), see _range_plan
JUNK = 7.0                             # what rows at and beyond kv_len hold: finite, of another scale, inside the f16x2 range
LDS_LIMIT = 160 * 1024

TAG_2, TAG_2Q, TAG_2W, TAG_3, TAG_F32 = "wavlm_attention2", "wavlm_attention2q", "wavlm_attention2w", "wavlm_attention3", "wavlm_attention"
TAGS = (TAG_2, TAG_2Q, TAG_2W, TAG_3, TAG_F32)
QB2 = (("KNNSVC_ATT_QB", "2"), ("KNNSVC_ATT_NW", "4"))       # the knobs that force a schedule of the f16x2 route
NW8 = (("KNNSVC_ATT_QB", "2"), ("KNNSVC_ATT_NW", "8"))
QB1 = (("KNNSVC_ATT_QB", "1"),)
F32 = (("KNNSVC_ATTENTION", "fp32"),)                        # read once per process (or reload): these rows run in attention_fp32_child.py


# ------------------------------------------------------------------ the reference
def scores(q, k, gate, table, b, h, dtype, rows=None):
    """[len(rows), T] score matrix of batch row b, head h, in `dtype` (no key is excluded here)."""
    T = q.shape[1]
    i = torch.arange(T) if rows is None else torch.as_tensor(rows, dtype=torch.long)
    j = torch.arange(T)
    s = (q[b, i, h].to(dtype) @ k[b, :, h].to(dtype).T) / 8
    return s + gate[b, i, h].to(dtype)[:, None] * table[h].to(dtype)[j[None, :] - i[:, None] + T - 1]


def clamp_len(kv_len, b, T):
    return T if kv_len is None else min(max(int(kv_len[b]), 1), T)


def attention_ref(q, k, v, gate, table, kv_len, dtype, rows=None, chunk=256):
    """-> [B, len(rows), H, 64] in `dtype` (rows: the queries to evaluate, default all T): explicit scores, keys
    j >= clamp(kv_len[b], 1, T) excluded, softmax as exp(s - max) / sum, then P @ V.  Query chunks keep the long rows small."""
    B, T, H, D = q.shape
    rows = torch.arange(T) if rows is None else torch.as_tensor(rows, dtype=torch.long)
    out = torch.zeros(B, len(rows), H, D, dtype=dtype)
    for b in range(B):
        tk = clamp_len(kv_len, b, T)
        for h in range(H):
            vv = v[b, :tk, h].to(dtype)
            for c0 in range(0, len(rows), chunk):
                s = scores(q, k, gate, table, b, h, dtype, rows[c0:c0 + chunk])[:, :tk]
                p = torch.exp(s - s.max(-1, keepdim=True).values)
                out[b, c0:c0 + chunk, h] = (p / p.sum(-1, keepdim=True)) @ vv
    return out


def bucket_table(table, T, n):
    """The columns of a length-T table that a launch at exactly n frames indexes: [H, 2n - 1]."""
    return table[:, T - n:T - n + 2 * n - 1].contiguous()


# ------------------------------------------------------------------ the dispatcher, asked (ops.attention_route launches nothing)
ROUTE_KNOBS = ("KNNSVC_ATTENTION", "KNNSVC_ATT_QB", "KNNSVC_ATT_NW")


def route(B, T, H, wide=False, env=(), out_split=False, kv_split=False):
    """-> (tag, bytes of LDS) knnsvc_wavlm_attention takes under the knobs `env` and no other, as the library itself answers;
    KnnSvcError where it refuses the call.  The environment is put back afterwards."""
    from knn_svc_amd import ops
    old = {k: os.environ.pop(k, None) for k in ROUTE_KNOBS}
    try:
        os.environ.update(dict(env))
        ops.reload_knobs()
        return ops.attention_route(B, T, H, out_split, kv_split, wide)
    finally:
        for k, v in old.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v
        ops.reload_knobs()


@functools.lru_cache(maxsize=None)
def longest_T(tag):
    """The largest T (B = H = 1) the dispatcher gives to `tag` under the knobs that force it: one frame more is refused — or,
    from the eight-wave kernel, handed to the four-wave one."""
    from knn_svc_amd._lib import KnnSvcError

    def fits(T):
        try:
            return route(1, T, 1, tag == TAG_3, FORCE_ENV[tag])[0] == tag
        except KnnSvcError:
            return False
    lo, hi = 129, 258
    assert fits(lo)
    while fits(hi):
        lo, hi = hi, 2 * hi
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if fits(mid) else (lo, mid)
    return lo


def schedules(T):
    """Every f16x2 schedule a length admits: (knobs, tag)."""
    out = []
    for env in (QB1, QB2, NW8):
        tag = route(1, T, 1, env=env)[0]
        if tag not in [t for _, t in out]:
            out.append((env, tag))
    return out


# ------------------------------------------------------------------ the rows
@dataclass(frozen=True)
class Case:
    id: str
    tag: str                    # what ops.last_attention_kernel() must say
    B: int
    T: int
    H: int
    kv_len: tuple | None = None  # per batch row, as handed to the kernel (values < 1 and > T are clamped there)
    family: str = "model"
    kv_split: bool = False      # K and V handed over in the f16x2 split layout
    out_split: bool = False     # output written in the f16x2 split layout (read back through ops.split_unpack)
    wide: bool = False          # flag bit 2: the bf16x3 kernel
    env: tuple = ()             # the knobs this row sets; every other knob of the dispatcher is unset
    sample: bool = False        # long rows: err over the first and last 160 queries and every 97th between, not all of them
    seed: int = 0

    @property
    def route(self) -> str:
        return {TAG_3: "bf16x3", TAG_F32: "fp32"}.get(self.tag, "f16x2")

    @property
    def fp32_child(self) -> bool:
        return dict(self.env).get("KNNSVC_ATTENTION") == "fp32"

    def rows(self):
        if not self.sample:
            return torch.arange(self.T)
        T = self.T
        return torch.unique(torch.cat([torch.arange(160), torch.arange(160, T - 160, 97), torch.arange(T - 160, T)]))


def _junk(x, kv_len):
    if kv_len is not None:
        T = x.shape[1]
        for b in range(x.shape[0]):
            x[b, clamp_len(kv_len, b, T):] = JUNK
    return x


def family_inputs(family, B, T, H, seed=0):
    """Seeded q, k, v [B, T, H, 64], gate [B, T, H], table [H, 2T - 1] (float32) of an input family:
      model       q, k, v ~ 0.5 N(0, 1), gate U(0, 2), table N(0, 1);
      peaked      q, k ~ 4 N(0, 1) (scores of standard deviation 16), table 30 N(0, 1): the softmax is almost one-hot;
      rising      k_j = (j + 1) u, q = 2 u (|u| = 1): the score grows by 0.25 per key, 8 per 32-key step, against a bias below
                  0.8 — every step raises the running maximum (alpha < 1);
      falling     k_j = (T - j) u: the first step holds the maximum, alpha == 1 in every later step (the ballot skips the rescale);
      onelane     falling, but query min(37, T - 1) has q = -2 u: in every later step exactly that query has alpha != 1;
      uniform     all keys equal, table 0: every weight is 1 / T, the output is the mean of V and l_run reaches T;
      cancelling  uniform weights over V = +-1000 (alternating along the keys) + N(0, 1): the sum cancels to O(1 / sqrt(T));
      small       q, k, v ~ 2^-10 N(0, 1): the lo plane of the scale-16 split is subnormal;
      limit_kv    k, v uniform in +-0.9 A2_LIMIT with one element at the bound, q ~ N(0, 1) scaled so that the scores have
                  standard deviation 4;     limit_q: q uniform in +-4 A2_LIMIT, k scaled likewise, v ~ 0.5 N(0, 1);
      limit_kv100 / limit_q100: the same times 100 on the large operands (and / 100 on the small one): beyond f16x2, the
                  point of `wide` and of the fp32 route."""
    g = torch.Generator().manual_seed(1000 * T + 10 * H + B + 7919 * seed + sum(map(ord, family)))
    n = lambda *s: torch.randn(*s, generator=g)
    u01 = lambda *s: torch.rand(*s, generator=g)
    q, k, v = 0.5 * n(B, T, H, HD), 0.5 * n(B, T, H, HD), 0.5 * n(B, T, H, HD)
    gate, table = 2 * u01(B, T, H), n(H, 2 * T - 1)
    if family == "model":
        pass
    elif family == "peaked":
        q, k, v, table = 8 * q, 8 * k, 2 * v, 30 * table
    elif family in ("rising", "falling", "onelane"):
        u = torch.full((HD,), 0.125)
        ramp = torch.arange(1, T + 1, dtype=torch.float32) if family == "rising" else torch.arange(T, 0, -1, dtype=torch.float32)
        k = (ramp[:, None] * u)[None, :, None, :].expand(B, T, H, HD).clone()
        q = (2 * u)[None, None, None, :].expand(B, T, H, HD).clone()
        if family == "onelane":
            q[:, min(37, T - 1)] = -2 * u
        v, table = 2 * v, 0.1 * table.clamp(-4, 4)
    elif family in ("uniform", "cancelling"):
        k = k[:, :1].expand(B, T, H, HD).clone()
        table = torch.zeros_like(table)
        v = 2 * v
        if family == "cancelling":
            sign = 1 - 2 * (torch.arange(T) % 2).float()
            v = v + 1000 * sign[None, :, None, None]
    elif family == "small":
        q, k, v = q * 2.0 ** -9, k * 2.0 ** -9, v * 2.0 ** -9
    elif family.startswith("limit_"):
        big = 100.0 if family.endswith("100") else 1.0
        uni = lambda lim: (2 * u01(B, T, H, HD) - 1) * lim
        if family.startswith("limit_kv"):
            lim = 0.9 * A2_LIMIT * big
            k, v = uni(lim), uni(lim)
            k[0, 0, 0, 0], v[0, 0, 0, 1] = lim, -lim
            q = n(B, T, H, HD) * (4.0 / (lim / 3 ** 0.5))          # q . k / 8: 64 terms of std s_q lim / sqrt(3) -> std 4
        else:
            lim = 4 * A2_LIMIT * big
            q = uni(lim)
            q[0, 0, 0, 0] = lim
            k = n(B, T, H, HD) * (4.0 / (lim / 3 ** 0.5))
    else:
        raise ValueError(family)
    return q.contiguous(), k.contiguous(), v.contiguous(), gate.contiguous(), table.contiguous()


@functools.lru_cache(maxsize=None)
def inputs(case):
    """The row's operands, with JUNK in the q / k / v rows at and beyond each batch row's (clamped) kv_len."""
    q, k, v, gate, table = family_inputs(case.family, case.B, case.T, case.H, case.seed)
    return _junk(q, case.kv_len), _junk(k, case.kv_len), _junk(v, case.kv_len), gate, table


@functools.lru_cache(maxsize=None)
def yardstick(case):
    """-> (ref64 [B, rows, H, 64], e32, scale, valid): the float64 reference at case.rows(), e32 = max |float32 evaluation - ref64| and
    scale = max |v| over what counts, valid [B, rows] = the query rows below kv_len."""
    q, k, v, gate, table = inputs(case)
    rows = case.rows()
    ref = attention_ref(q, k, v, gate, table, case.kv_len, torch.float64, rows)
    r32 = attention_ref(q, k, v, gate, table, case.kv_len, torch.float32, rows)
    valid = torch.stack([rows < clamp_len(case.kv_len, b, case.T) for b in range(case.B)])
    e32 = float((r32.double() - ref).abs()[valid].max())
    scale = max(float(v[b, :clamp_len(case.kv_len, b, case.T)].abs().max()) for b in range(case.B))
    return ref, e32, scale, valid


T_EDGES = (1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 192, 193, 255, 256, 257, 333, 511, 512, 513)
KV_EDGES = (0, 1, 31, 32, 33, 64, 65, "T-1", "T", "T+5")
FAMILIES = ("model", "peaked", "rising", "falling", "onelane", "uniform", "cancelling", "small", "limit_kv", "limit_q")
SHORT = {TAG_2: "2", TAG_2Q: "2q", TAG_2W: "2w", TAG_3: "3", TAG_F32: "f32"}
ROUTE_ENV = {TAG_2: (), TAG_2Q: QB2, TAG_2W: NW8, TAG_3: (), TAG_F32: F32}
FORCE_ENV = dict(ROUTE_ENV, **{TAG_2: QB1})                  # the knobs under which a kernel is taken whatever the grid's size
# the rows at the longest T a kernel takes: what longest_T(tag) answers (tests/test_attention_cpu.py holds the two together)
LONGEST = {TAG_2: 15712, TAG_2Q: 15712, TAG_2W: 6240, TAG_3: 14112, TAG_F32: 16256}


def _kv(T, i, B):
    res = lambda e: {"T-1": T - 1, "T": T, "T+5": T + 5}.get(e, e)
    return tuple(res(KV_EDGES[(i + 3 * b) % len(KV_EDGES)]) for b in range(B))


def _table():
    cases = []
    add = lambda *a, **kw: cases.append(Case(*a, **kw))
    # T edges on every kernel: one 32-key step, the key tile, the 128 / 256 / 512-query workgroups, an odd step count.  B = 3 with
    # kv_len walking through KV_EDGES (every third row has none), H alternating 2 and 3; the split flags alternate on the f16x2 rows
    for tag in TAGS:
        for i, T in enumerate(T_EDGES):
            if tag in (TAG_2Q, TAG_2W) and T <= 128:
                continue
            f16 = tag in (TAG_2, TAG_2Q, TAG_2W)
            add(f"{SHORT[tag]}-T{T}", tag, 3, T, 2 + i % 2, None if i % 3 == 2 else _kv(T, i, 3), wide=tag == TAG_3, env=ROUTE_ENV[tag],
                kv_split=f16 and i % 2 == 1, out_split=f16 and i % 4 >= 2)
    # forced 64 queries per wave at T <= 128 lands on the 128-query kernel
    for T in (64, 128):
        add(f"2-forced-qb2-T{T}", TAG_2, 2, T, 2, (T, T - 1), env=QB2)
        add(f"2-forced-nw8-T{T}", TAG_2, 2, T, 2, (T - 1, T + 5), env=NW8)
    # one visible key in every batch row of a longer launch: the weight is 1 and every kernel returns that key's V row itself, so
    # e32 = 0 and the tolerance is the floor alone
    for tag in TAGS:
        add(f"{SHORT[tag]}-one-key-T129", tag, 3, 129, 2, (0, 1, 1), wide=tag == TAG_3, env=ROUTE_ENV[tag])
    # natural dispatch, no knobs: both sides of blocks128 >= 1536 and of blocks512 >= 512
    add("natural-47x129x16", TAG_2, 47, 129, 16)
    add("natural-48x129x16", TAG_2W, 48, 129, 16)
    add("natural-24x400x16", TAG_2Q, 24, 400, 16)
    add("natural-32x400x16", TAG_2W, 32, 400, 16)
    # a few H = 16 rows with lengths and flags, one per kernel
    for tag in TAGS:
        f16 = tag in (TAG_2, TAG_2Q, TAG_2W)
        add(f"{SHORT[tag]}-H16", tag, 2, 333, 16, (333 - 31, 65), wide=tag == TAG_3, env=ROUTE_ENV[tag], kv_split=f16, out_split=f16)
    # the LDS fallback of the eight-wave kernel, and the longest T every kernel accepts
    t2w = LONGEST[TAG_2W]
    add(f"2w-longest-T{t2w}", TAG_2W, 1, t2w, 1, env=NW8, sample=True)
    add(f"2q-lds-fallback-T{t2w + 1}", TAG_2Q, 1, t2w + 1, 1, env=NW8, sample=True)
    add(f"2-longest-T{LONGEST[TAG_2]}", TAG_2, 1, LONGEST[TAG_2], 1, env=QB1, sample=True)
    add(f"2q-longest-T{LONGEST[TAG_2Q]}", TAG_2Q, 1, LONGEST[TAG_2Q], 1, env=QB2, sample=True)
    add(f"3-longest-T{LONGEST[TAG_3]}", TAG_3, 1, LONGEST[TAG_3], 1, wide=True, sample=True)
    add(f"f32-longest-T{LONGEST[TAG_F32]}", TAG_F32, 1, LONGEST[TAG_F32], 1, env=F32, sample=True)
    # input families: T = 333 (eleven 32-key steps, the last tile has one; three ragged 128-query blocks), B = 2, the second batch
    # row one step short
    for tag in TAGS:
        fams = FAMILIES + (("limit_kv100", "limit_q100") if tag in (TAG_3, TAG_F32) else ())
        for fam in fams:
            if fam == "model":
                continue                                    # the T-edge rows
            add(f"{SHORT[tag]}-{fam}", tag, 2, 333, 2, (333, 333 - 31), family=fam, wide=tag == TAG_3, env=ROUTE_ENV[tag])
    return tuple(cases)


CASES = _table()

# bucketed against exact-length launch, per kernel: (id, tag, T, H, knobs, wide); n runs over BUCKET_N
BUCKET_T, BUCKET_N = 333, (332, 302, 65, 1)
BUCKETS = tuple((f"bucket-{SHORT[t]}", t, BUCKET_T, 2, ROUTE_ENV[t], t == TAG_3) for t in TAGS)
# a B = 3 launch against three B = 1 launches, per kernel
BATCHES = tuple((f"batch-{SHORT[t]}", t, 257, 3, (257, 200, 33), ROUTE_ENV[t], t == TAG_3) for t in TAGS)

# calls every route must refuse before anything is launched: (id, what the message says); tests/attention_child.py makes them
REFUSED = (("null-qkv", "null pointer"), ("null-gate", "null pointer"), ("null-table", "null pointer"), ("null-out", "null pointer"),
           ("T0", "bad sizes"), ("heads0", "bad sizes"), ("misaligned-qkv", "16-byte alignment"), ("misaligned-out", "16-byte alignment"))
SPLIT_REFUSED = ("wide-kv_split", "wide-out_split")              # flag bit 2 with a split layout (main child)
F32_SPLIT_REFUSED = ("fp32-kv_split", "fp32-out_split")          # the fp32 route with a split layout (fp32 child)
# one frame more than longest_T(tag) is refused ("T too long"), under the knobs that reach the kernel; the eight-wave kernel falls
# back to the four-wave one instead (the 2q-lds-fallback row)
TOO_LONG = {t: e for t, e in FORCE_ENV.items() if t != TAG_2W}
