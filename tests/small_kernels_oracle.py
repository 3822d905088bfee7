"""References and case generators for the small kernels between the stages (csrc/elementwise.hip, csrc/synth.hip and absmax /
mean3 / axpy of csrc/conv_gemm.hip): what tests/small_kernels_child.py compares the GPU with and tests/test_small_kernels_cpu.py
checks on the CPU.  numpy and torch on the CPU only: nothing here opens the GPU (conv0_subs asks the library's host-only route entry).

Every reference is written over its arguments' dtype: float64 arguments give the fp64 reference, float32 arguments the "plain
fp32 evaluation" whose error against the fp64 reference is the yardstick of the child's third comparison rule.  Where oracle/
has the operation (synth_ref.additive_synth, sine_excitation, harmonic_amps, prematch_ref.amp_ratio) that is used and nothing is
restated; sine_excitation64 is the one exception: the oracle casts the wrapped phase to fp32 before the sine (as the model
does), so a reference that is fp64 to the end needs the cast left out."""
import math

import numpy as np
import torch
import torch.nn.functional as F


def rng(*key):
    """A generator seeded by the case's own parameters: a case's inputs do not depend on which cases ran before it."""
    g = torch.Generator()
    g.manual_seed(abs(hash(tuple(int(k) for k in key))) % (2 ** 31))
    return g


# ------------------------------------------------------------------ references (dtype of the arguments = dtype of the arithmetic)
def gelu(x):
    return 0.5 * x * (1.0 + torch.erf(x * (1.0 / math.sqrt(2.0))))


def layernorm(x, gamma, beta, with_gelu=False, eps=1e-5):
    """Two-pass LayerNorm over the last axis (biased variance, eps inside the root), then the erf GELU."""
    mean = x.mean(-1, keepdim=True)
    d = x - mean
    var = (d * d).mean(-1, keepdim=True)
    y = d / torch.sqrt(var + eps) * gamma + beta
    return gelu(y) if with_gelu else y


def conv0(x, w, gamma, beta, k, stride, rows=None):
    """GELU(LN_channels(conv1d(x[B, L], w[C, k], stride))) -> [B * T, C]; ``rows``: only these flat (b * T + t) rows."""
    B, L = x.shape
    T = (L - k) // stride + 1
    fr = x.unfold(1, k, stride)                                # [B, T, k]
    assert fr.shape[1] == T
    fr = fr.reshape(B * T, k)
    if rows is not None:
        fr = fr[rows]
    return layernorm(fr @ w.T, gamma, beta, True)


def conv0_length(T, k, stride):
    """The input length of the conv0 cases: T output rows and stride - 1 samples more, so that the length ends off the stride
    grid and the last staged span reaches past L."""
    return (T - 1) * stride + k + stride - 1


def gate(x, heads, w2, b2, grep_a):
    """WavLM's gated relative position multiplier per (row, head): x [rows, >= heads * 64], w2 [2, 64], b2 [2], grep_a [heads]."""
    xh = x[:, :heads * 64].reshape(x.shape[0], heads, 64)
    ga = torch.sigmoid(xh @ w2[0] + b2[0])
    gb = torch.sigmoid(xh @ w2[1] + b2[1])
    return ga * (gb * grep_a[None, :heads] - 1.0) + 2.0


def mask_rows(x, batches, T, dim, lens):
    """x [batches * T, ld]: columns < dim of rows t >= lens[b] become zero, everything else keeps its bits."""
    out = x.clone()
    for b in range(batches):
        if lens[b] < T:
            out[b * T + max(int(lens[b]), 0):(b + 1) * T, :dim] = 0.0
    return out


def reflect_index(n, pad):
    j = np.arange(-pad, n + pad)
    j = np.abs(j)
    return np.where(j >= n, 2 * (n - 1) - j, j)


def reflect_pad(x, pad, extra=0):
    """[n] -> [n + 2 pad + extra]: reflection without repeating the edge sample, zeros behind."""
    out = torch.zeros(x.numel() + 2 * pad + extra, dtype=x.dtype)
    out[:x.numel() + 2 * pad] = x[torch.from_numpy(reflect_index(x.numel(), pad))]
    return out


def reflect_pad_batch(x_flat, offs, pad, stride):
    out = torch.zeros(len(offs) - 1, stride, dtype=x_flat.dtype)
    for b in range(len(offs) - 1):
        n = offs[b + 1] - offs[b]
        out[b, :n + 2 * pad] = reflect_pad(x_flat[offs[b]:offs[b + 1]], pad)
    return out


def complex_mag(reim, bins):
    """[rows, >= 2 bins] (real parts, then imaginary parts) -> [rows, bins] magnitudes."""
    return torch.hypot(reim[:, :bins], reim[:, bins:2 * bins])


def harmonic_amps64(spec, f0, n_harm):
    """The oracle with an fp64 spectrum: the bin is chosen from the fp32 f0 in fp32 (that choice IS the specification), the
    interpolation and the scaling run in fp64."""
    from oracle import synth_ref
    return synth_ref.harmonic_amps(spec.double(), f0.float(), n_harm)


def harmonic_positions(f0, n_harm, bins):
    """What the harmonic kernels decide per (frame, harmonic), in fp32 and in their order of operations ->
    (pos before rounding, gi, src before its clamp, i0); voiced frames only (f0 == 0 takes the unvoiced rule)."""
    f = np.asarray(f0, np.float32)[:, None]
    k = np.arange(1, n_harm + 1, dtype=np.float32)[None, :]
    nb = np.float32(bins * 8)
    pos = np.minimum(((f * k) * np.float32(2.0)) * nb / np.float32(16000.0), nb).astype(np.float32)
    gi = np.rint(pos).astype(np.int64)
    src = (gi.astype(np.float32) + np.float32(0.5)) * np.float32(0.125) - np.float32(0.5)
    i0 = np.maximum(src, 0).astype(np.int64)
    voiced = np.broadcast_to(f != 0, pos.shape)
    return pos[voiced], gi[voiced], src[voiced], i0[voiced]


def weighted_gather(idx, w, pool):
    """sum_j w[i, j] * pool[idx[i, j]]"""
    return (pool[idx.reshape(-1)].reshape(idx.shape[0], idx.shape[1], -1) * w[..., None]).sum(1)


def uniform_gather_f32(idx, pool, mean_mode):
    """The kernel's fp32 operations in its order, one rounding each: mode 0 sums x * (1.0f / k), mode 1 sums x and divides by k."""
    k = idx.shape[1]
    g = pool.float()[idx.reshape(-1)].reshape(idx.shape[0], k, -1)
    kf = torch.tensor(float(k), dtype=torch.float32)
    wj = torch.tensor(1.0, dtype=torch.float32) / kf
    acc = g[:, 0] if mean_mode else g[:, 0] * wj
    for j in range(1, k):
        acc = acc + (g[:, j] if mean_mode else g[:, j] * wj)
    return acc / kf if mean_mode else acc


def round_f16(x):
    return x.half().float()


def abs_bits_max(x):
    """max |x| the way a range slot orders it: by the bits of |x|, so that NaN sorts above inf -> the float with those bits."""
    b = np.ascontiguousarray(x.detach().cpu().numpy(), dtype=np.float32).view(np.uint32) & np.uint32(0x7FFFFFFF)
    return np.array([b.max() if b.size else 0], np.uint32).view(np.float32)[0]


def mean3_f32(a, b, c, div):
    return (c + (b + a)) / torch.tensor(div, dtype=torch.float32)


def axpy_f32(x, alpha, out, accumulate):
    v = x * torch.tensor(alpha, dtype=torch.float32)
    return out + v if accumulate else v


def sine_excitation64(f0, sr=16000, hop=320):
    """synth_ref.sine_excitation without its fp32 cast of the wrapped phase: f0 [N] -> [N * hop] in fp64."""
    om = torch.cumsum(torch.repeat_interleave(f0.double(), hop) / sr, 0)
    return torch.sin(2 * math.pi * (om - torch.round(om)))


def prenet(exc, pw, pb):
    """The generator's sin_prenet: Conv1d(1 -> n_ch, k = 3, padding 1) over the excitation -> [L, n_ch]."""
    return F.conv1d(exc[None, None], pw[:, None, :], pb, padding=1)[0].T


# ------------------------------------------------------------------ case generators
LN_DIMS = (4, 36, 252, 256, 260, 512, 516, 768, 1024, 1028, 2048)
LN_ROWS = (1, 3, 17)


def layernorm_inputs(rows, dim, kind="normal"):
    """normal: the distribution of test_gpu_kernels.test_layernorm_gelu (x ~ 3 N(0,1) + 1, gamma and beta ~ N(0,1)); constant:
    every row one value; offset: 1000 + N(0,1) / 100."""
    g = rng(1, rows, dim)
    x = torch.randn(rows, dim, generator=g) * 3 + 1
    ga, be = torch.randn(dim, generator=g), torch.randn(dim, generator=g)
    if kind == "constant":
        x = torch.full((rows, dim), 3.0) * torch.arange(1, rows + 1)[:, None]
    elif kind == "offset":
        x = 1000.0 + torch.randn(rows, dim, generator=g) * 0.01
    return x, ga, be


C0_CHANNELS = (64, 128, 256, 512)
C0_TAPS = ((10, 5), (3, 2), (16, 8), (1, 1), (11, 5))
C0_T = (1, 63, 64, 65, 130)
C0_BATCHES = (1, 3)
C0_MULTISPAN = dict(batches=3072, channels=64, k=10, stride=5, T=130)


def conv0_cases():
    return [dict(channels=c, k=k, stride=s, T=T, batches=B) for c in C0_CHANNELS for k, s in C0_TAPS for T in C0_T for B in C0_BATCHES]


def conv0_inputs(batches, channels, k, stride, T):
    g = rng(2, batches, channels, k, stride, T)
    x = torch.randn(batches, conv0_length(T, k, stride), generator=g)
    w = torch.randn(channels, k, generator=g) / math.sqrt(k)
    return x, w, torch.randn(channels, generator=g), torch.randn(channels, generator=g)


def conv0_subs(T, batches):
    """The spans of 64 rows a workgroup of knnsvc_wavlm_conv0 walks for this launch, as the dispatcher itself answers
    (ops.conv0_route: host code, nothing is launched)."""
    from knn_svc_amd import ops
    return ops.conv0_route(batches, T)[1]


def conv0_dispatch_rule():
    """(the spans a workgroup walks on the multi-span route, the workgroup count from which the dispatcher takes it), found by
    asking it about inputs of 64 frames: one workgroup per batch item on either route, so the workgroup count is the batch."""
    subs = conv0_subs(64, 65535)
    return subs, next(b for b in range(1, 65536) if conv0_subs(64, b) > 1)


def gate_weights():
    """The seeded gate parameters test_gpu_kernels.test_attention_and_gate uses -> (w2 [2, 64], b2 [2], grep_a [16])."""
    from knn_svc_amd import config as C, synthetic as S
    cfg = dict(C.WAVLM_LARGE, encoder_layers=1)
    p = "encoder.layers.0.self_attn."
    sd = S.seeded_state([s for s in S.wavlm_param_spec(cfg) if s[0].startswith(p[:-1])], 3)
    w8, b8 = sd[p + "grep_linear.weight"], sd[p + "grep_linear.bias"]
    return (torch.stack([w8[:4].sum(0), w8[4:].sum(0)]).contiguous(), torch.stack([b8[:4].sum(), b8[4:].sum()]),
            sd[p + "grep_a"].reshape(-1).contiguous())


HARM_BINS = (1, 8, 63, 200, 257)
HARM_ROWS = (1, 5)
HARM_N = (1, 49, 64, 65, 130)
HARM_F0 = (0.0, 102.5, 12.5, 2.5, 10.0, 163.26, 1047.0, 7999.0, 8000.0, 0.0)     # two chunks of five frames, each with an unvoiced one


def reim_inputs(rows, bins):
    """[rows, 2 bins]: magnitudes log-uniform over 1e-18 .. 1e18 per component, random signs; about one component in six is an exact
    zero (so some bins are exactly zero, some purely real or imaginary).  Neighbouring bins differ by orders of magnitude."""
    g = rng(3, rows, bins)
    e = torch.rand(rows, 2 * bins, generator=g) * 36 - 18
    v = torch.pow(torch.tensor(10.0, dtype=torch.float64), e.double()).float()
    v = v * (torch.randint(0, 2, v.shape, generator=g) * 2 - 1)
    v[torch.rand(v.shape, generator=g) < 1 / 6] = 0.0
    if bins > 1:
        v[0, 1] = 0.0; v[0, bins + 1] = 0.0                                        # one bin exactly zero
    return v


def harmonic_cases():
    """(bins, n_harm, f0 [rows]): one-frame calls take the f0 values in turn, five-frame calls the two halves of HARM_F0."""
    out, turn = [], 0
    for bins in HARM_BINS:
        for n_harm in HARM_N:
            out.append((bins, n_harm, np.array([HARM_F0[1 + turn % 8]], np.float32)))
            turn += 1
            out.append((bins, n_harm, np.array(HARM_F0[:5], np.float32)))
            out.append((bins, n_harm, np.array(HARM_F0[5:], np.float32)))
    return out


SYNTH_N = (1, 2, 3, 5, 50, 1100)
SYNTH_HOP = (320, 7, 400)
SYNTH_H = (1, 49)


def synth_inputs(N, H, n_ch, zero_f0=False):
    """f0 [N] with unvoiced frames, fundamentals up to 1000 Hz (harmonics of a 49-harmonic stack pass Nyquist from 163.3 Hz on) and
    one frame above Nyquist itself; amp = rand * 0.02 (test_gpu_kernels.test_additive_synth's golden, tests/gen_golden.py);
    prenet weights ~ N(0,1) as in that test."""
    g = rng(4, N, H, n_ch)
    f0 = 80.0 + torch.rand(N, generator=g) * 920.0
    f0[torch.rand(N, generator=g) < 0.25] = 0.0
    if N >= 3:
        f0[1] = 0.0; f0[2] = 171.3
    if N >= 5:
        f0[4] = 8100.0
    if N == 1:
        f0[0] = 220.5
    if zero_f0:
        f0 = torch.zeros(N)
    amp = torch.rand(N, H, generator=g) * 0.02
    return f0, amp, torch.randn(n_ch, 3, generator=g), torch.randn(n_ch, generator=g)


def synth_cases():
    """(mode, N, hop, H, n_ch, want_exc, zero_f0): every N x hop x H in mode 0 and every N x hop in mode 1, n_ch and want_exc taking
    turns so that each of their four combinations occurs in both modes; then the all-zero tracks."""
    out, turn = [], 0
    for mode, hs in ((0, SYNTH_H), (1, (0,))):
        for N in SYNTH_N:
            for hop in SYNTH_HOP:
                for H in hs:
                    out.append((mode, N, hop, H, (1, 32)[turn & 1], bool(turn & 2), False))
                    turn += 1
        out.append((mode, 5, 320, 49 if mode == 0 else 0, 32, True, True))
        out.append((mode, 50, 7, 1 if mode == 0 else 0, 1, True, True))
    return out


SYNTH_DYN_N = (50, 1100)


def synth_dyn_counts(N):
    return (0, 1, N - 3, N, N + 5)


# One launch more than the list above: the smallest bucket of the vocoder's 25 frames that lies past 1024 frames, with a count
# below 1024.  The frame-phase prefix takes ceil(frames / 1024) frames per thread; it grouped the bucket's 1025 frames in pairs
# where the exact launch sums its 1010 one by one, and the fp64 sums' other order moved 70 of 323 200 samples by an fp32 ulp.
SYNTH_DYN_CROSSING = (1025, 1010)


MEAN3_N = (4, 1028, 4 * (256 * 4 * 4096 + 3))        # the last: one float4 group of three past a full pass of the capped grid
MEAN3_GRID_CAP = 4096                                # blocks, each of 256 threads taking 4 float4 groups per pass (csrc/conv_gemm.hip)

GATHER_K = (1, 3, 4, 8)
GATHER_DIM = (1, 49, 255, 1030)


def gather_inputs(k, dim, nq=7, npool=50):
    """idx with repeats inside a row and the rows 0 and npool - 1; positive weights that sum to one, as smooth_weights gives."""
    g = rng(5, k, dim)
    pool = torch.randn(npool, dim, generator=g)
    idx = torch.randint(0, npool, (nq, k), generator=g)
    idx[0, :] = 0
    idx[1, :] = npool - 1
    if k > 1:
        idx[2, 1] = idx[2, 0]
    w = torch.softmax(torch.randn(nq, k, generator=g), -1)
    return idx, w, pool


AMP_NQ, AMP_K, AMP_BINS = (1, 5), (1, 4, 8), (1, 63, 257)


def amp_ratio_inputs(nq, k, bins, npool=40):
    """rand * 3 spectra as in test_gpu_kernels.test_round_f16_and_amp_ratio; pool row 7 is silent and the first index names it."""
    g = rng(6, nq, k, bins)
    sq, sp = torch.rand(nq, bins, generator=g) * 3, torch.rand(npool, bins, generator=g) * 3
    sp[7] = 0
    idx = torch.randint(0, npool, (nq, k), generator=g)
    idx[0, 0] = 7
    return sq, sp, idx


ROUND_N = (1, 3, 5, 1027)


def round_f16_inputs(n):
    """test_gpu_kernels.test_round_f16_and_amp_ratio's values: N(0,1) times logspace(-9, 5): fp16 subnormals to overflow."""
    g = rng(7, n)
    return torch.randn(n, generator=g) * torch.logspace(-9, 5, 37)[torch.arange(n) % 37]
