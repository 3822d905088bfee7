"""CPU: the yardsticks and the route table of the attention tests (tests/attention_oracle.py) — the reference against torch's SDPA
and against the oracle's bias path, the table against the dispatcher itself (asked through its host-only route entry, at every
row and on both sides of every boundary of its rules), and every input family against the branch of the flash step it is named for."""
import os

import pytest
import torch
import torch.nn.functional as F

from tests import attention_oracle as A


def _sdpa64(q, k, v, gate, table, kv_len):
    """F.scaled_dot_product_attention in float64 with the bias and the key mask written out as one additive mask."""
    B, T, H, _ = q.shape
    i, j = torch.arange(T)[:, None], torch.arange(T)[None, :]
    bias = gate.double().permute(0, 2, 1)[..., None] * table.double()[:, j - i + T - 1][None]           # [B, H, T, T]
    for b in range(B):
        bias[b, :, :, A.clamp_len(kv_len, b, T):] = float("-inf")
    sh = lambda x: x.double().permute(0, 2, 1, 3)
    return F.scaled_dot_product_attention(sh(q), sh(k), sh(v), attn_mask=bias).permute(0, 2, 1, 3)


@pytest.mark.parametrize("B,T,H,kv_len", [(1, 1, 1, None), (2, 33, 2, (0, 40)), (3, 65, 3, (64, 65, 1)), (2, 130, 2, (129, 31))])
def test_reference_equals_sdpa_in_fp64(B, T, H, kv_len):
    q, k, v, gate, table = A.family_inputs("model", B, T, H, seed=1)
    ref = A.attention_ref(q, k, v, gate, table, kv_len, torch.float64, chunk=50)
    want = _sdpa64(q, k, v, gate, table, kv_len)
    assert ref.dtype == torch.float64 and float((ref - want).abs().max()) < 1e-13
    rows = torch.tensor([0, T // 2, T - 1])
    assert float((A.attention_ref(q, k, v, gate, table, kv_len, torch.float64, rows) - ref[:, rows]).abs().max()) < 1e-14
    r32 = A.attention_ref(q, k, v, gate, table, kv_len, torch.float32)
    assert r32.dtype == torch.float32 and 0 < float((r32.double() - ref).abs().max()) < 1e-5 or T == 1


def test_reference_equals_the_oracles_bias_path():
    """The inputs of test_attention_and_gate (T = 333, B = 2, H = 16): oracle/wavlm_ref's gate and [H, T, T] position bias as SDPA's
    additive mask, against attention_ref on the kernel's operands (the gate per query and head, the [H, 2T - 1] table)."""
    from knn_svc_amd import config as C, synthetic as S
    from oracle import wavlm_ref
    cfg = dict(C.WAVLM_LARGE, encoder_layers=1)
    H, E, T, B = 16, 1024, 333, 2
    sd = S.seeded_state([s for s in S.wavlm_param_spec(cfg) if s[0].startswith("encoder.layers.0.self_attn")], 3)
    xn = torch.randn(T, B, E, generator=torch.Generator().manual_seed(2))
    p = "encoder.layers.0.self_attn."
    gate_ref = wavlm_ref.gate(sd, cfg, 0, xn)                                    # [B, H, T, 1]
    pb = wavlm_ref.position_bias(sd, cfg, T)                                     # [H, T, T]
    lin = lambda n: F.linear(xn, sd[p + n + "_proj.weight"], sd[p + n + "_proj.bias"])
    sh = lambda t: t.reshape(T, B * H, 64).transpose(0, 1).reshape(B, H, T, 64)
    q, k, v = sh(lin("q")), sh(lin("k")), sh(lin("v"))
    want = F.scaled_dot_product_attention(q.double(), k.double(), v.double(), attn_mask=gate_ref.double() * pb[None].double())
    table = sd[p + "relative_attention_bias.weight"][wavlm_ref.rel_bucket_table(T, 320, 800)].T.contiguous()
    bthd = lambda x: x.permute(0, 2, 1, 3).contiguous()
    got = A.attention_ref(bthd(q), bthd(k), bthd(v), gate_ref[..., 0].permute(0, 2, 1).contiguous(), table, None, torch.float64)
    assert float((got - bthd(want)).abs().max()) < 1e-12


def test_bucket_slice_is_the_exact_length_table():
    from oracle import wavlm_ref
    emb = torch.randn(320, 3, generator=torch.Generator().manual_seed(4))
    T = A.BUCKET_T
    table = emb[wavlm_ref.rel_bucket_table(T, 320, 800)].T.contiguous()
    for n in A.BUCKET_N:
        assert torch.equal(A.bucket_table(table, T, n), emb[wavlm_ref.rel_bucket_table(n, 320, 800)].T)
    q, k, v, gate, tb = A.family_inputs("model", 1, 40, 2, seed=9)               # ... and indexes the same scores
    n = 17
    a = A.attention_ref(q, k, v, gate, tb, (n,), torch.float64)[:, :n]
    b = A.attention_ref(q[:, :n], k[:, :n], v[:, :n], gate[:, :n], A.bucket_table(tb, 40, n), None, torch.float64)
    assert float((a - b).abs().max()) < 1e-14


# ------------------------------------------------------------------ the table
def test_ids_are_unique_and_every_tag_has_rows():
    ids = [c.id for c in A.CASES]
    assert len(ids) == len(set(ids))
    for tag in A.TAGS:
        assert sum(c.tag == tag for c in A.CASES) >= 3, tag
    assert {t for _, t, *_ in A.BUCKETS} == set(A.TAGS) == {t for _, t, *_ in A.BATCHES}


def test_rows_cover_what_the_issue_lists():
    for tag in A.TAGS:
        ts = {c.T for c in A.CASES if c.tag == tag and c.family == "model"}
        assert ts >= {T for T in A.T_EDGES if T > 128 or tag not in (A.TAG_2Q, A.TAG_2W)}, tag
        fams = {c.family for c in A.CASES if c.tag == tag}
        assert fams >= set(A.FAMILIES), (tag, set(A.FAMILIES) - fams)
        if tag in (A.TAG_3, A.TAG_F32):
            assert fams >= {"limit_kv100", "limit_q100"}
    for route in ("f16x2", "bf16x3", "fp32"):
        seen = set()
        for c in A.CASES:
            if c.route == route and c.kv_len:
                seen |= {("T-1" if n == c.T - 1 else "T" if n == c.T else "T+5" if n == c.T + 5 else n) for n in c.kv_len}
        assert seen >= set(A.KV_EDGES), (route, set(A.KV_EDGES) - seen)
    assert any(c.kv_split and c.out_split for c in A.CASES) and any(c.kv_split != c.out_split for c in A.CASES)
    assert all(not (c.kv_split or c.out_split) for c in A.CASES if c.route != "f16x2")
    natural = {(c.B, c.T, c.H): c.tag for c in A.CASES if c.id.startswith("natural")}
    assert natural == {(47, 129, 16): A.TAG_2, (48, 129, 16): A.TAG_2W, (24, 400, 16): A.TAG_2Q, (32, 400, 16): A.TAG_2W}
    assert all(c.env == () for c in A.CASES if c.id.startswith("natural"))


def test_the_dispatcher_agrees_with_the_table():
    for c in A.CASES:
        tag, lds = A.route(c.B, c.T, c.H, c.wide, c.env, c.out_split, c.kv_split)
        assert tag == c.tag, c.id
        assert 0 < lds <= A.LDS_LIMIT, c.id


NW4 = (("KNNSVC_ATT_NW", "4"),)
QB2_ONLY = (("KNNSVC_ATT_QB", "2"),)


@pytest.mark.parametrize("B,T,H,env,tag", [
    # ceil(T / 128) H B = 1535 / 1536: 64 queries per wave from two rounds of the resident workgroups on
    (1, 640, 307, NW4, A.TAG_2), (1, 768, 256, NW4, A.TAG_2Q), (1, 640, 307, (), A.TAG_2), (1, 768, 256, (), A.TAG_2W),
    # ... and never at T <= 128, whatever forces it
    (2, 128, 2, A.QB2, A.TAG_2), (2, 129, 2, A.QB2, A.TAG_2Q), (2, 128, 2, A.NW8, A.TAG_2), (2, 129, 2, A.NW8, A.TAG_2W),
    (1536, 128, 1, (), A.TAG_2), (768, 129, 1, (), A.TAG_2W),
    # ceil(T / 512) H B = 511 / 512 with KNNSVC_ATT_NW unset: eight waves from two rounds of one workgroup per CU on
    (73, 3584, 1, (), A.TAG_2Q), (256, 1024, 1, (), A.TAG_2W), (73, 3584, 1, QB2_ONLY, A.TAG_2Q), (256, 1024, 1, QB2_ONLY, A.TAG_2W),
])
def test_the_dispatch_rules_at_their_boundaries(B, T, H, env, tag):
    assert A.route(B, T, H, env=env)[0] == tag
    if not env:
        assert ((T + 127) // 128 * H * B, (T + 511) // 512 * H * B) in ((1535, 614), (1536, 512), (1536, 1536), (1536, 768), (2044, 511), (2048, 512))


def test_flags_and_modes():
    from knn_svc_amd._lib import KnnSvcError
    assert A.route(2, 333, 2, wide=True)[0] == A.TAG_3                           # flag bit 2 on the f16x2 default
    assert A.route(2, 333, 2, env=(("KNNSVC_ATTENTION", "bf16x3"),))[0] == A.TAG_3
    assert A.route(2, 333, 2, wide=True, env=A.F32)[0] == A.TAG_F32              # the fp32 route has the range anyway
    for kw in (dict(wide=True), dict(env=A.F32)):
        for split in (dict(out_split=True), dict(kv_split=True)):
            with pytest.raises(KnnSvcError, match="only implemented by the f16x2 kernel"):
                A.route(2, 333, 2, **kw, **split)
    for B, T, H in ((0, 8, 2), (4, 0, 2), (4, 8, 0), (65536, 8, 2), (4, 8, 65536)):
        with pytest.raises(KnnSvcError, match="bad sizes"):
            A.route(B, T, H)
    assert {A.route(1, 129, 1, t == A.TAG_3, A.FORCE_ENV[t])[0] for t in A.TAGS} == set(A.TAGS)


def test_longest_lengths():
    from knn_svc_amd._lib import KnnSvcError
    assert A.longest_T(A.TAG_2W) == 6240 and {t: A.longest_T(t) for t in A.TAGS} == A.LONGEST
    for tag in A.TAGS:
        T, wide, env = A.longest_T(tag), tag == A.TAG_3, A.FORCE_ENV[tag]
        got, lds = A.route(1, T, 1, wide, env)
        assert got == tag and lds <= A.LDS_LIMIT < lds + 8                   # a frame more is two more entries of the bias table
        if tag == A.TAG_2W:
            assert A.route(1, T + 1, 1, wide, env)[0] == A.TAG_2Q            # falls back to the four-wave kernel
        else:
            with pytest.raises(KnnSvcError, match="T too long for the LDS bias table"):
                A.route(1, T + 1, 1, wide, env)
        assert any(c.tag == tag and c.T == T and c.B == c.H == 1 for c in A.CASES), tag
    t = A.longest_T(A.TAG_2W)
    assert A.schedules(t + 1) == [(A.QB1, A.TAG_2), (A.QB2, A.TAG_2Q)] and len(A.schedules(129)) == 3 and len(A.schedules(128)) == 1
    assert A.schedules(t) == [(A.QB1, A.TAG_2), (A.QB2, A.TAG_2Q), (A.NW8, A.TAG_2W)]


def test_asking_leaves_the_environment_as_it_was(monkeypatch):
    monkeypatch.setenv("KNNSVC_ATT_QB", "1")
    monkeypatch.delenv("KNNSVC_ATT_NW", raising=False)
    assert A.route(2, 333, 2, env=A.NW8)[0] == A.TAG_2W
    assert os.environ["KNNSVC_ATT_QB"] == "1" and "KNNSVC_ATT_NW" not in os.environ


# ------------------------------------------------------------------ the families reach their branches
def _step_maxima(fam, T=333, b=0, h=1):
    """[T, steps]: per query the maximum of the float64 reference scores over every 32-key step."""
    q, k, v, gate, table = A.family_inputs(fam, 2, T, 2)
    s = A.scores(q, k, gate, table, b, h, torch.float64)
    pad = torch.full((T, (-T) % 32), float("-inf"), dtype=torch.float64)
    return torch.cat([s, pad], 1).view(T, -1, 32).max(-1).values


def test_rising_raises_the_maximum_in_every_step():
    m = _step_maxima("rising")
    assert m.shape[1] == 11 and bool((m[:, 1:] > m[:, :-1] + 1.0).all())          # alpha = exp(m_old - m_new) < e^-1 throughout


def test_falling_never_raises_it_after_the_first():
    m = _step_maxima("falling")
    assert bool((m[:, 1:] < m[:, :1] - 1.0).all())                               # the running maximum stays: alpha == 1 exactly


def test_onelane_has_exactly_one_query_that_does():
    m = _step_maxima("onelane")
    run = torch.cummax(m, 1).values
    raised = (run[:, 1:] > run[:, :-1]).any(1)
    assert raised.nonzero().flatten().tolist() == [37]
    assert bool((m[37, 1:] > m[37, :-1] + 1.0).all())                             # ... in every step, the late ones included
    others = torch.arange(333) != 37
    assert bool((m[others][:, 1:] < m[others][:, :1] - 1.0).all())
    assert 37 // 32 == 1 and 37 % 32 == 5                                         # one lane pair of wave 1


def test_uniform_and_cancelling_have_equal_weights():
    for fam in ("uniform", "cancelling"):
        q, k, v, gate, table = A.family_inputs(fam, 2, 333, 2)
        s = A.scores(q, k, gate, table, 1, 0, torch.float64)
        assert float((s - s[:, :1]).abs().max()) < 1e-12          # (a blocked matmul may round the columns of equal keys apart)
    ref = A.attention_ref(q, k, v, gate, table, None, torch.float64)
    assert float(v.abs().min()) > 990 and float(ref.abs().max()) < 1000 / 333 + 1   # +-1000 cancels to the last (odd) key / T + noise
    assert bool((v[:, 0::2] > 0).all()) and bool((v[:, 1::2] < 0).all())


def test_small_and_limit_lie_where_stated():
    q, k, v, _, _ = A.family_inputs("small", 2, 333, 2)
    for x in (q, k, v):
        # 16 x = hi + lo: hi keeps 11 bits, so |lo| <= 2^-11 |16 x| — below fp16's smallest normal 2^-14 wherever |x| < 2^-7
        assert float(x.abs().max()) < 2.0 ** -7 and 2.0 ** -11 < float(x.abs().mean()) < 2.0 ** -10
    lim = A.A2_LIMIT
    from knn_svc_amd.wavlm import WavLMEncoder
    assert lim == WavLMEncoder.A2_LIMIT
    for fam, big in (("limit_kv", 1.0), ("limit_kv100", 100.0)):
        q, k, v, gate, table = A.family_inputs(fam, 2, 333, 2)
        assert float(k.abs().max()) == pytest.approx(0.9 * lim * big) and float(v.abs().max()) == pytest.approx(0.9 * lim * big)
        assert float(k.abs().max()) < lim * big and float(q.abs().max()) < 0.05 / big
        assert 2.0 < float(A.scores(q, k, torch.zeros_like(gate), table, 0, 0, torch.float64).std()) < 8.0
    for fam, big in (("limit_q", 1.0), ("limit_q100", 100.0)):
        q, k, v, gate, table = A.family_inputs(fam, 2, 333, 2)
        assert float(q.abs().max()) == pytest.approx(4 * lim * big) and float(q.abs().max()) < 5 * lim * big     # _range_plan: qb < 5 lim
        assert float(k.abs().max()) < 0.01 / big
        assert 2.0 < float(A.scores(q, k, torch.zeros_like(gate), table, 0, 0, torch.float64).std()) < 8.0
    # the f16x2 operands stay inside fp16: K' = 16 K, V' = 16 V, Q' = 16 log2(e) / 8 Q
    assert 16 * 0.9 * lim < 65504 and 16 * 1.4426950408889634 / 8 * 4 * lim < 65504


def test_junk_sits_behind_kv_len_only():
    c = next(c for c in A.CASES if c.id == "2-T65")
    q, k, v, _, _ = A.inputs(c)
    for b in range(c.B):
        n = A.clamp_len(c.kv_len, b, c.T)
        for x in (q, k, v):
            assert bool((x[b, n:] == A.JUNK).all()) and not bool((x[b, :n] == A.JUNK).any())
    ref, e32, scale, valid = A.yardstick(c)
    assert valid.sum() == sum(A.clamp_len(c.kv_len, b, c.T) for b in range(c.B)) and 0 < e32 < 1e-5 and scale < 4
