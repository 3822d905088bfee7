"""CPU: what tests/small_kernels_child.py relies on, shown without a GPU.
  references       each fp64 reference of tests/small_kernels_oracle.py agrees with torch's own operator (or the project's oracle) at
                   the level of that operator's fp32 error
  case generators  the inputs reach the branches they are meant to reach: conditions, not measurements
  refusals         every entry point of the small kernels refuses what its KN_REQUIRE lines forbid before anything is launched (the
                   pointers are dummies that are never dereferenced), with a nonzero code and its own name in knnsvc_last_error()"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import small_kernels_oracle as O


def _lib():
    import __graft_entry__ as g
    g.build()
    from knn_svc_amd import _lib
    return _lib.load()


def _close(a, b, tol):
    return float((a.double() - b.double()).abs().max()) <= tol


# ------------------------------------------------------------------ references
@pytest.mark.parametrize("dim", [4, 260, 2048])
def test_layernorm_and_gelu_reference_agree_with_torch(dim):
    x, ga, be = O.layernorm_inputs(17, dim)
    ref = O.layernorm(x.double(), ga.double(), be.double(), True)
    assert _close(ref, F.gelu(F.layer_norm(x.double(), (dim,), ga.double(), be.double(), 1e-5)), 1e-13)
    assert _close(ref, F.gelu(F.layer_norm(x, (dim,), ga, be, 1e-5)), 1e-5)                  # fp32 torch: the project's bound
    assert _close(O.layernorm(x, ga, be, True), ref, 1e-5)                                    # the plain fp32 evaluation (the yardstick)
    assert _close(O.gelu(x.double()), F.gelu(x.double()), 1e-14)
    xc, ga, be = O.layernorm_inputs(3, dim, "constant")
    assert torch.equal(O.layernorm(xc, ga, be), be[None].expand(3, dim))


@pytest.mark.parametrize("k,stride", O.C0_TAPS)
def test_conv0_reference_agrees_with_conv1d(k, stride):
    x, w, ga, be = O.conv0_inputs(3, 64, k, stride, 65)
    want = F.conv1d(x.double()[:, None], w.double()[:, None], stride=stride).transpose(1, 2).reshape(-1, 64)
    want = F.gelu(F.layer_norm(want, (64,), ga.double(), be.double(), 1e-5))
    ref = O.conv0(x.double(), w.double(), ga.double(), be.double(), k, stride)
    assert ref.shape == (3 * 65, 64) and _close(ref, want, 1e-12)
    rows = torch.tensor([0, 64, 65, 194])
    assert torch.equal(O.conv0(x.double(), w.double(), ga.double(), be.double(), k, stride, rows), ref[rows])
    assert _close(O.conv0(x, w, ga, be, k, stride), ref, 1e-5)


def test_gate_reference_agrees_with_the_wavlm_oracle():
    from knn_svc_amd import config as C, synthetic as S
    from oracle import wavlm_ref
    cfg = dict(C.WAVLM_LARGE, encoder_layers=1)
    sd = S.seeded_state([s for s in S.wavlm_param_spec(cfg) if s[0].startswith("encoder.layers.0.self_attn")], 3)
    xn = torch.randn(7, 2, 1024, generator=O.rng(1))
    want = wavlm_ref.gate(sd, cfg, 0, xn)[..., 0]                                  # [B, H, T]
    w2, b2, a = O.gate_weights()
    got = O.gate(xn.transpose(0, 1).reshape(14, 1024).double(), 16, w2.double(), b2.double(), a.double())
    assert _close(got.reshape(2, 7, 16).permute(0, 2, 1), want, 1e-5)
    assert O.gate(xn[:, 0].double(), 12, w2.double(), b2.double(), a.double()).shape == (7, 12)


@pytest.mark.parametrize("n,pad", [(2, 1), (201, 200), (1000, 200), (257, 0)])
def test_reflect_pad_reference_is_torchs_reflect_mode(n, pad):
    x = torch.randn(n, generator=O.rng(n))
    assert torch.equal(O.reflect_pad(x, pad), F.pad(x[None, None], (pad, pad), mode="reflect")[0, 0] if pad else x)
    got = O.reflect_pad(x, pad, 112)
    assert got.numel() == n + 2 * pad + 112 and not got[n + 2 * pad:].any()


def test_reflect_pad_batch_and_mask_rows_references():
    lens, offs = [201, 1000, 202], [0, 201, 1201, 1403]
    x = torch.randn(1403, generator=O.rng(2))
    out = O.reflect_pad_batch(x, offs, 200, 1500)
    for b, n in enumerate(lens):
        assert torch.equal(out[b, :n + 400], F.pad(x[None, None, offs[b]:offs[b + 1]], (200, 200), mode="reflect")[0, 0])
        assert not out[b, n + 400:].any()
    m = torch.randn(4 * 50, 96, generator=O.rng(3))
    got = O.mask_rows(m, 4, 50, 64, [0, 50, 17, 77])
    keep = torch.ones(200, 96, dtype=torch.bool)
    keep[0:50, :64] = False
    keep[100 + 17:150, :64] = False
    assert torch.equal(got[keep], m[keep]) and not got[~keep].any()


def test_complex_mag_reference_and_its_inputs():
    v = O.reim_inputs(5, 257)
    ref = O.complex_mag(v.double(), 257)
    assert torch.equal(ref, torch.hypot(v.double()[:, :257], v.double()[:, 257:]))
    rel = ((torch.hypot(v[:, :257], v[:, 257:]).double() - ref).abs() / ref.clamp_min(1e-300)).max()
    assert float(rel) < 2.0 ** -23
    nz = ref[ref > 0]
    assert float(nz.min()) < 1e-15 and float(nz.max()) > 1e15 and bool((ref == 0).any()) and bool(torch.isfinite(ref.float()).all())
    ratio = (ref[:, 1:] / ref[:, :-1].clamp_min(1e-30)).log10().abs()
    assert float(ratio.median()) > 1.0                     # neighbouring bins differ by orders of magnitude: a wrong bin shows


def test_harmonic_reference_is_the_oracle_with_the_fp32_bin_choice():
    from oracle import synth_ref
    spec = O.complex_mag(O.reim_inputs(5, 200), 200)
    f0 = torch.tensor(O.HARM_F0[:5])
    a, b = O.harmonic_amps64(spec, f0, 49), synth_ref.harmonic_amps(spec, f0, 49)
    rel = (a - b.double()).abs() / a.abs().clamp_min(1e-300)
    assert a.dtype == torch.float64 and float(rel.max()) < 4 * 2.0 ** -23 and torch.equal(a == 0, b == 0)


def test_sine_and_synth_references_agree_with_the_oracle():
    from oracle import synth_ref
    f0, amp, pw, pb = O.synth_inputs(50, 49, 32)
    for hop in (7, 320):
        ref = O.sine_excitation64(f0, hop=hop)
        assert _close(ref, synth_ref.sine_excitation(f0[None, :, None], hop=hop)[0, 0], 4e-7)       # the fp32 cast of a phase of up to pi
    wave = synth_ref.additive_synth(f0[None, :, None], amp[None])[0, :, 0]
    assert torch.equal(O.prenet(wave, pw, pb), F.conv1d(wave[None, None], pw[:, None], pb, padding=1)[0].T)
    assert bool((f0 == 0).any()) and float((f0 * 49).max()) > 8000 and float(f0.max()) > 8000


def test_gather_round_and_fold_references():
    idx, w, pool = O.gather_inputs(4, 49)
    ref = O.weighted_gather(idx, w.double(), pool.double())
    assert _close(ref, sum(w[:, j, None].double() * pool.double()[idx[:, j]] for j in range(4)), 1e-15)
    assert int(idx.min()) == 0 and int(idx.max()) == pool.shape[0] - 1 and int(idx[2, 0]) == int(idx[2, 1])
    for k in O.GATHER_K:
        idx, w, pool = O.gather_inputs(k, 255)
        m0, m1 = O.uniform_gather_f32(idx, pool, 0), O.uniform_gather_f32(idx, pool, 1)
        assert _close(m1, pool[idx.reshape(-1)].reshape(7, k, -1).double().mean(1), 1e-6)
        assert k & (k - 1) or torch.equal(m0, m1)               # a power-of-two k: 1.0f / k and the division are both exact scalings
    x = O.round_f16_inputs(1027)
    assert bool(torch.isinf(O.round_f16(x)).any()) and bool(((O.round_f16(x) == 0) & (x != 0)).any())
    assert np.isnan(O.abs_bits_max(torch.tensor([1.0, float("nan"), float("inf")])))
    assert O.abs_bits_max(torch.tensor([-3.0, 2.0])) == 3.0 and O.abs_bits_max(torch.zeros(0)) == 0.0


# ------------------------------------------------------------------ case generators
def test_harmonic_cases_reach_every_branch():
    halves = pad = neg = last = second_pass = 0
    for bins, n_harm, f0 in O.harmonic_cases():
        pos, gi, src, i0 = O.harmonic_positions(f0, n_harm, bins)
        halves += int(((pos - np.floor(pos)) == 0.5).sum())
        pad += int((gi >= bins * 8).sum())
        neg += int(((src < 0) & (gi < bins * 8)).sum())
        last += int(((i0 == bins - 1) & (gi < bins * 8) & (bins > 1)).sum())
        second_pass += int(n_harm > 64)
    assert halves >= 4 and pad >= 1 and neg >= 1 and last >= 1 and second_pass >= 1, (halves, pad, neg, last, second_pass)
    assert any((f0 == 0).any() for _, _, f0 in O.harmonic_cases())
    assert {len(f0) for _, _, f0 in O.harmonic_cases()} == set(O.HARM_ROWS)
    used = np.unique(np.concatenate([f0 for _, _, f0 in O.harmonic_cases()]))
    assert set(used.tolist()) == set(np.array(O.HARM_F0, np.float32).tolist())


def test_exact_halves_round_to_even_in_the_reference():
    pos, gi, _, _ = O.harmonic_positions(np.array([2.5], np.float32), 5, 200)
    assert pos.tolist() == [0.5, 1.0, 1.5, 2.0, 2.5] and gi.tolist() == [0, 1, 2, 2, 2]


def test_conv0_lengths_end_off_the_stride_grid_and_the_multispan_case_is_the_smallest():
    for c in O.conv0_cases() + [O.C0_MULTISPAN]:
        L = O.conv0_length(c["T"], c["k"], c["stride"])
        assert (L - c["k"]) // c["stride"] + 1 == c["T"]
        assert c["stride"] == 1 or (L - c["k"]) % c["stride"] == c["stride"] - 1
        m0 = (c["T"] - 1) // 64 * 64                              # the last span stages 63 stride + k samples from row m0 on
        assert c["T"] % 64 == 0 or m0 * c["stride"] + 63 * c["stride"] + c["k"] > L
    subs, least = O.conv0_dispatch_rule()
    m = O.C0_MULTISPAN
    assert (subs, least) == (8, 3072)
    assert O.conv0_subs(m["T"], m["batches"]) == subs and O.conv0_subs(m["T"], m["batches"] - 1) == 1
    assert -(-m["T"] // 64) == 3                                # three spans: both LDS buffers, and a break in the fourth round
    assert all(O.conv0_subs(c["T"], c["batches"]) == 1 for c in O.conv0_cases())
    assert len(O.conv0_cases()) == 200


def test_layernorm_synth_and_mean3_cases_reach_their_branches():
    assert {d % 256 != 0 for d in O.LN_DIMS} == {True, False} and max(O.LN_DIMS) > 1024 and min(O.LN_DIMS) == 4
    assert 17 in O.LN_ROWS and 17 % 4 and 17 % 2                 # a wave takes 4, 2 or 1 rows, a workgroup four times that: 17 fills neither
    cases = O.synth_cases()
    for mode in (0, 1):
        mine = [c for c in cases if c[0] == mode and not c[6]]
        assert {(c[1], c[2]) for c in mine} == {(n, h) for n in O.SYNTH_N for h in O.SYNTH_HOP}
        assert {(c[4], c[5]) for c in mine} == {(1, False), (1, True), (32, False), (32, True)}
        assert sum(c[6] for c in cases if c[0] == mode) == 2
    assert {c[3] for c in cases if c[0] == 0} == set(O.SYNTH_H) and max(O.SYNTH_N) > 1024
    n4 = O.MEAN3_N[-1] // 4
    assert -(-n4 // (256 * 4)) > O.MEAN3_GRID_CAP and n4 - O.MEAN3_GRID_CAP * 256 * 4 == 3


# ------------------------------------------------------------------ refusals
D = 256                     # a dummy, 16-byte aligned, never dereferenced: every call below fails before a read or a launch


def _refusals(lib):
    N = None
    return {
        "layernorm: dim 6": lambda: lib.knnsvc_layernorm(D, 4, 6, 8, D, D, 0, D, 8, N),
        "layernorm: dim 2052": lambda: lib.knnsvc_layernorm(D, 4, 2052, 2052, D, D, 0, D, 2052, N),
        "layernorm: split with dim 36": lambda: lib.knnsvc_layernorm(D, 4, 36, 36, D, D, 2, D, 64, N),
        "layernorm: misaligned x": lambda: lib.knnsvc_layernorm(D + 4, 4, 64, 64, D, D, 0, D, 64, N),
        "layernorm: misaligned out": lambda: lib.knnsvc_layernorm(D, 4, 64, 64, D, D, 0, D + 4, 64, N),
        "wavlm_conv0: 96 channels": lambda: lib.knnsvc_wavlm_conv0(D, 1, 400, D, 96, 10, 5, D, D, D, 0, N),
        "wavlm_conv0: k 17": lambda: lib.knnsvc_wavlm_conv0(D, 1, 400, D, 64, 17, 5, D, D, D, 0, N),
        "wavlm_conv0: stride 9": lambda: lib.knnsvc_wavlm_conv0(D, 1, 400, D, 64, 10, 9, D, D, D, 0, N),
        "wavlm_conv0: split at 64 channels": lambda: lib.knnsvc_wavlm_conv0(D, 1, 400, D, 64, 10, 5, D, D, D, 1, N),
        "wavlm_conv0: L < k": lambda: lib.knnsvc_wavlm_conv0(D, 1, 9, D, 64, 10, 5, D, D, D, 0, N),
        "wavlm_gate: head_dim 32": lambda: lib.knnsvc_wavlm_gate(D, 5, 16, 32, 1024, D, D, D, D, 0, N),
        "wavlm_gate: 17 heads": lambda: lib.knnsvc_wavlm_gate(D, 5, 17, 64, 1088, D, D, D, D, 0, N),
        "mask_rows: dim 6": lambda: lib.knnsvc_mask_rows(D, 2, 50, 6, 8, D, N),
        "reflect_pad: n == pad": lambda: lib.knnsvc_reflect_pad(D, 5, 5, D, N),
        "reflect_pad: n < pad": lambda: lib.knnsvc_reflect_pad(D, 3, 7, D, N),
        "reflect_pad_batch: stride == 2 pad": lambda: lib.knnsvc_reflect_pad_batch(D, D, 2, 200, D, 400, N),
        "reflect_pad_batch: stride < 2 pad": lambda: lib.knnsvc_reflect_pad_batch(D, D, 2, 200, D, 399, N),
        "spec_harm: 4097 bins": lambda: lib.knnsvc_spec_harm(D, 5, 4097, 2 * 4097, D, 49, D, D, N),
        "spec_harm: ld < 2 bins": lambda: lib.knnsvc_spec_harm(D, 5, 200, 399, D, 49, D, D, N),
        "weighted_gather: mean_mode 2": lambda: lib.knnsvc_weighted_gather(D, None, 5, 4, D, 64, 64, 2, D, N),
        "round_f16: misaligned x": lambda: lib.knnsvc_round_f16(D + 4, 8, D, N),
        "round_f16: misaligned out": lambda: lib.knnsvc_round_f16(D, 8, D + 4, N),
        "amp_ratio: ld_q < bins": lambda: lib.knnsvc_amp_ratio(D, 199, D, 200, 40, D, 5, 4, 200, D, N),
        "amp_ratio: ld_pool < bins": lambda: lib.knnsvc_amp_ratio(D, 200, D, 199, 40, D, 5, 4, 200, D, N),
        "additive_synth: H 1025": lambda: lib.knnsvc_additive_synth(D, D, 50, 1025, 320, 16000, 0, D, D, 32, D, 32, N, D, N, N),
        "additive_synth: mode 0 without amp": lambda: lib.knnsvc_additive_synth(D, N, 50, 49, 320, 16000, 0, D, D, 32, D, 32, N, D, N, N),
        "additive_synth: N hop >= 2^31": lambda: lib.knnsvc_additive_synth(D, D, 6710887, 49, 320, 16000, 0, D, D, 32, D, 32, N, D, N, N),
        "mean3: n 6": lambda: lib.knnsvc_mean3(D, D, D, 6, 3.0, D, N, N, 0, N),
        "mean3: div 0": lambda: lib.knnsvc_mean3(D, D, D, 8, 0.0, D, N, N, 0, N),
        "axpy: n 6": lambda: lib.knnsvc_axpy(D, 6, 1.0, 0, D, N),
        "absmax: ld < cols": lambda: lib.knnsvc_absmax(D, 5, 37, 36, D, N),
    }


def test_every_entry_point_refuses_what_it_forbids_before_launching():
    lib = _lib()
    assert 6710887 * 320 >= 2 ** 31 > 6710886 * 320
    for what, call in _refusals(lib).items():
        name = what.split(":")[0]
        rc = call()
        msg = lib.knnsvc_last_error()
        assert rc != 0 and name.encode() + b":" in msg, (what, rc, msg)


def test_the_refusals_cover_every_entry_point_the_child_calls():
    names = {w.split(":")[0] for w in _refusals(None)}
    assert names == {"layernorm", "wavlm_conv0", "wavlm_gate", "mask_rows", "reflect_pad", "reflect_pad_batch", "spec_harm",
                     "weighted_gather", "round_f16", "amp_ratio", "additive_synth", "mean3", "axpy", "absmax"}
