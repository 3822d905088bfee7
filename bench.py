"""Headline benchmark: end-to-end kNN-SVC conversion throughput (xRT) on MI355X.

    python bench.py --gpus N --steps K --warmup W          (N > 1: launched by torch.distributed.run, one rank per GPU;
                                                            without RANK in the environment it starts its N ranks itself)
        [--full]                 everything else the benchmark measures (see below); a plain run only sets up, warms up,
                                 times the K steps and prints the headline line
        [--dump-outputs DIR]     after the timed steps: the waveform the last timed step returned, DIR/waveform.npy (float32)

One *step* = one cold conversion per rank on synthetic inputs already resident in HBM:
WavLM-Large (6 layers) encode of a 10-minute target pool shard (20 x 30 s) and a 30 s source,
STFT + harmonic amplitudes, cosine kNN top-32 (pool sharded over ranks, RCCL all-gather merge),
f0 shift / re-rank, concat re-selection, two Adam smoothness loops, additive synth, conditioned
HiFi-GAN generator ('mix', post_opt_0.2).  Weights are seeded random tensors of the real
architectures (no network for the released checkpoints).  value = source seconds converted by all
ranks / wall time of the slowest rank.

Extra objects on the JSON line, with --full only (each takes passes of its own after the timed steps):
  config.sequential_ms_per_step — the same K steps again with conversions one after the other (latency);
  value_long_adam — the same K steps with both Adam smoothness loops forced to 2000 iterations;
  knn          — the kNN stage's rate and roofline, from the eager pass below;
  other_configs — BASELINE cfg 5 (one GPU's share) and cfg 3 through the product entry points (rank 0, N = 1 only);
  roofline     — the dominant kernel (conv_gemm2quad_kernel<Gemm2QuadS>: implicit GEMM, 256x256 block tiles of
                 v_mfma_f32_16x16x32_f16, fp32 emulated as three fp16 MFMAs per product): algorithmic fp32 FLOP
                 (2*M*N*K per launch) / HIP-event time of those launches, against the dense fp16 matrix peak / 3
                 (and, for reference, the 157.3 TFLOP/s fp32 peak);
  cpu_baseline — the CPU oracle (a port of the reference's --device cpu path) timed on this box's
                 host cores on a bounded sample of the same workload (rank 0, N = 1 only); the sample is
                 scaled to the full step, so the object carries "extrapolated": true and the per-stage seconds.
"""
import argparse
import json
import os
import sys
import time


def _self_launch_ranks():
    """`python bench.py --gpus N` with N > 1 and no RANK in the environment (the shape of the driver's one-GPU command with another
    N): start the N ranks ourselves.  This runs before anything is imported that could touch the GPU; the ranks are CHILD processes
    of `python -m torch.distributed.run` (never an exec of this process), their stdout / stderr are ours, so rank 0's JSON line is
    relayed as it is, and a failing rank makes this process exit non-zero."""
    if "RANK" in os.environ or "--gpus" not in " ".join(sys.argv[1:]):
        return
    ap = argparse.ArgumentParser(add_help=False)
    ap.add_argument("--gpus", type=int, default=1)
    n = ap.parse_known_args()[0].gpus
    if n <= 1:
        return
    import socket
    import subprocess
    with socket.socket() as s:                 # a free rendezvous port on the loopback interface
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n}", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    print(f"bench.py: --gpus {n} without RANK: launching {n} ranks: {' '.join(cmd[1:8])} ...", file=sys.stderr, flush=True)
    sys.exit(subprocess.run(cmd, env=env).returncode)


if __name__ == "__main__":
    _self_launch_ranks()

import numpy as np
import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")

from knn_svc_amd import config as C, dist as kdist, ops, synthetic as S      # noqa: E402
from knn_svc_amd.matching import match_features, side_features, side_features_many               # noqa: E402
from knn_svc_amd.pipeline import LanePipeline                                 # noqa: E402
from knn_svc_amd.vocoder import Vocoder                                       # noqa: E402
from knn_svc_amd.wavlm import WavLMEncoder, cat_rows                          # noqa: E402

FP32_MFMA_PEAK_TFLOPS = 157.3          # MI355X_MICROARCH.md: dense fp32 matrix peak
BF16_MFMA_PEAK_TFLOPS = 2500.0         # MI355X_MICROARCH.md: dense bf16 matrix peak (no sparsity)
BF16X3_PEAK_TFLOPS = BF16_MFMA_PEAK_TFLOPS / 6.0   # six bf16 MFMAs per fp32-accurate product (KNNSVC_GEMM=bf16x3)
F16X2_PEAK_TFLOPS = BF16_MFMA_PEAK_TFLOPS / 3.0    # three fp16 MFMAs per fp32-accurate product (default; fp16 rate = bf16 rate)
SRC_SECONDS = 30
LONG_ADAM_ITERS = 2000
POOL_CLIPS = 20                        # x 30 s = 10 minutes per rank


class GemmTimer:
    """HIP-event timing of every conv_gemm launch that can reach a candidate for "the dominant kernel" (the library
    reports which kernel it dispatched: Q256S = conv_gemm2quad_kernel<Gemm2QuadS>, the dominant one since round 2;
    F128 / F128a2 = conv_gemm2_kernel<Gemm2Tile<128,128,..>>), on the stream it is launched on, plus its algorithmic FLOP."""

    def __init__(self):
        self.records = []
        self.enabled = False
        self.all_variants = False
        # candidates for "the dominant kernel": both instantiations of conv_gemm2_kernel<Gemm2Tile<128,128,...>> (A fp32 / A
        # pre-split) count as one kernel, conv_gemm2quad_kernel<Gemm2QuadS> (long-K launches) as another; summary() reports the
        # one with more time in the step and carries the other along as `secondary`
        self.families = {"f16x2": (("F128", "F128a2"), ("Q256S",), ("Q256",)), "bf16x3": (("H128",),), "fp32": (("G128v8",),)}[ops.gemm_mode()]
        self.dominant = tuple(t for fam in self.families for t in fam)
        self.fam_bytes = {}
        self.dom_bytes = 0
        self._orig = ops.conv_gemm

    def install(self):
        orig = self._orig

        def wrapped(x, w, out, **kw):
            # only launches that can reach the dominant kernel (n > 64, 32-channel slabs) get an event pair, unless
            # --stages asked for the full table: event records around the many small launches would slow the eager pass
            cand = kw["n"] > 64 and kw["cin"] % 32 == 0
            if kw.get("defer") is not None or not (self.enabled and (cand or self.all_variants)):      # (deferred: launched later, as part of one grid)
                return orig(x, w, out, **kw)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            r = orig(x, w, out, **kw)
            e1.record()
            var = ops.last_conv_kernel()          # the library says which kernel it dispatched (F128a2, W64, G128v8, ...)
            if not (var in self.dominant or self.all_variants):
                return r
            z = kw.get("batches", 1) * kw.get("groups", 1)
            K = kw["cin"] * kw.get("taps", 1)
            flop = 2.0 * kw["m"] * kw["n"] * K * z
            t_in = kw.get("t_in") or kw["m"]
            self.records.append((e0, e1, flop, (kw["m"], kw["n"], K, z), var))
            if var in self.dominant:      # algorithmic floats moved: A read once (not im2col-expanded) + W + output
                self.fam_bytes[var] = self.fam_bytes.get(var, 0) + z * (t_in * kw["cin"] + kw["n"] * K + kw["m"] * kw["n"])
            return r
        ops.conv_gemm = wrapped

    def summary(self):
        """(tags, launches, ms, flop, floats moved) of every kernel family, most time first."""
        out = []
        for fam in self.families:
            recs = [r for r in self.records if r[4] in fam]
            if recs:
                out.append((fam, len(recs), sum(r[0].elapsed_time(r[1]) for r in recs), sum(r[2] for r in recs),
                            sum(self.fam_bytes.get(t, 0) for t in fam)))
        return sorted(out, key=lambda t: -t[2])


STRONG = False                         # --scaling strong: ONE 10-minute pool split over the ranks, one replicated source


def make_inputs(rank, dev):
    n = SRC_SECONDS * C.SAMPLE_RATE
    if STRONG:                         # same source everywhere; rank r holds its contiguous share of the SAME 20 pool clips
        src, sf0 = S.synth_clip(n, seed=1000)
        lo, hi = kdist.contiguous_share(POOL_CLIPS)
        pool = [S.synth_clip(30 * C.SAMPLE_RATE, seed=2000 + i) for i in range(lo, hi)]
    else:
        src, sf0 = S.synth_clip(n, seed=1000 + rank)
        pool = [S.synth_clip(30 * C.SAMPLE_RATE, seed=2000 + 100 * rank + i) for i in range(POOL_CLIPS)]
    g = lambda a: torch.from_numpy(a).to(dev)
    return g(src), g(sf0 * 1.3), [g(w) for w, _ in pool], [g(f) for _, f in pool]      # audio AND f0 tracks resident in HBM


STAGES = {}


class stage:
    """optional per-stage HIP-event timing (--stages), printed to stderr; not part of the contract line"""
    on = False

    def __init__(self, name):
        self.name = name

    def __enter__(self):
        if stage.on:
            self.e0 = torch.cuda.Event(enable_timing=True); self.e0.record()

    def __exit__(self, *a):
        if stage.on:
            e1 = torch.cuda.Event(enable_timing=True); e1.record()
            STAGES.setdefault(self.name, []).append((self.e0, e1))


_CONV = [0]                            # conversions started so far (the same count on every rank): who owns the next back half


def step_front(enc, src, sf0, pool_w, pool_f0, max_batch):
    """Encoder (+ STFT / harmonic amplitudes on a second stream) -> sharded kNN -> all-gathers."""
    # The encoder is enqueued first (its first kernels are long, so the host runs ahead); STFT / harmonic
    # amplitudes only need the raw audio and run on a second stream next to it.
    main = torch.cuda.current_stream()
    from knn_svc_amd.matching import _side_stream
    side = _side_stream(src.device)                      # the partner stream of whatever stream the front half runs on (created once per stream)
    side.wait_stream(main)
    with stage("wavlm"):
        feats = enc.encode_many(pool_w + [src], max_batch=max_batch)
    with torch.cuda.stream(side):
        with stage("side_features"):
            # one batched pass over the source and the 20 pool clips (matching.side_features_many), as get_complete_spk_pool does
            sides = side_features_many([src] + pool_w, [sf0] + pool_f0, [1500] * (1 + len(pool_w)))
            qf0 = sides[0][0]
            Pf0_loc = torch.cat([t[0] for t in sides[1:]]).contiguous()
            Ph_loc = torch.cat([t[1] for t in sides[1:]]).contiguous()
    qf = feats[-1]
    assert qf.shape[0] == 1500
    P_loc = cat_rows(feats[:-1]).contiguous()          # no copy: the clips of one batch lie back to back in the encoder's output
    main.wait_stream(side)
    for t in (qf0, Pf0_loc, Ph_loc):
        t.record_stream(main)
    if STRONG:
        # fixed pool, row-sharded in file order (uneven: 20 clips do not divide by 8); the replicated source is searched
        # once per shard and every rank needs the merged lists -> all-gather merge (dist.sharded_knn(replicated=True))
        rank, ws = kdist.world()
        base, rem = divmod(POOL_CLIPS, ws)
        counts = [1500 * (base + (1 if r < rem else 0)) for r in range(ws)]
        with stage("knn"):
            nn32, _ = kdist.sharded_knn(qf, P_loc, C.KNN_K, replicated=True, counts=counts)
        # ONE rank owns the back half (match + generator) of a conversion, and the owner rotates: conversion i belongs to
        # rank i mod ws, which alone receives the pool rows (point-to-point, no replication) — the other ranks go straight on
        # to the front half of conversion i + 1.  Per rank and conversion: 1/ws of the encoder + 1/ws of a back half.
        owner = _CONV[0] % ws
        _CONV[0] += 1
        with stage("gather"):
            P = kdist.gather_rows_var(P_loc, counts, owner)
            Pf0 = kdist.gather_rows_var(Pf0_loc, counts, owner)
            Ph = kdist.gather_rows_var(Ph_loc, counts, owner)
        if rank != owner:
            return None
        return dict(qf=qf, qf0=qf0, P=P, Pf0=Pf0, Ph=Ph, nn32=nn32)
    # The pool all-gathers start now and travel under the local kNN search; waited for below.  Two collectives, not three: f0 and
    # harmonics go as one [Np, 1 + 49] message — every collective the searching stream has to WAIT for costs the scheduling latency of
    # a kernel on RCCL's stream next to a busy chip (tools/bench_1rank_ab.sh), and these two are off the critical path altogether.
    P, wait_P = kdist.all_gather_rows_async(P_loc)
    side_loc = torch.cat([Pf0_loc[:, None], Ph_loc], 1) if dist.is_initialized() else None
    if side_loc is not None:
        side_all, wait_side = kdist.all_gather_rows_async(side_loc)
    with stage("knn"):
        # equal shards by construction: pass the sizes instead of letting sharded_knn read them back (a host sync)
        nn32, _ = kdist.sharded_knn(qf, P_loc, C.KNN_K, counts=[P_loc.shape[0]] * kdist.world()[1])
    with stage("gather"):
        wait_P()
        if side_loc is not None:
            wait_side()
            Pf0, Ph = side_all[:, 0].contiguous(), side_all[:, 1:].contiguous()
        else:
            Pf0, Ph = Pf0_loc, Ph_loc
    return dict(qf=qf, qf0=qf0, P=P, Pf0=Pf0, Ph=Ph, nn32=nn32)


def step_back(voc, f):
    """f0 shift / re-rank / concat re-selection / Adam weights / gathers -> additive synth + generator."""
    if f is None:                      # --scaling strong: another rank owns this conversion's back half
        return None
    with stage("match"):
        of, hw, s0, dbg = match_features(f["qf"], f["qf0"], f["P"], f["Pf0"], f["Ph"], "mix", "post_opt_0.2", nn32=f["nn32"],
                                         return_debug=True)
    with stage("vocoder"):
        y = voc.forward(of, s0, hw)
    step.last = dict(dbg, q=f["qf"], qf0=f["qf0"], P=f["P"], Pf0=f["Pf0"], Ph=f["Ph"], of=of, hw=hw, s0=s0)
    return y


def step(enc, voc, src, sf0, pool_w, pool_f0, max_batch):
    return step_back(voc, step_front(enc, src, sf0, pool_w, pool_f0, max_batch))


def run_steps(n, depth, enc, voc, src, sf0, pool_w, pool_f0, max_batch, pipe):
    """n conversions.  depth 1: one after the other on the current stream.  depth 2: through the package's
    stream scheduler (knn_svc_amd.pipeline.LanePipeline) — the back half of conversion i (match:
    single-workgroup recurrences on 2-4 CUs; vocoder) is enqueued on a second stream and runs while the front
    half of conversion i+1 (the encoder) fills the rest of the chip, the way bulk_match streams a list of
    sources.  Every conversion still does all of its work (cold pool).  (Tried in round 5, same box: the generator behind the
    NEXT encoder on the first stream instead of beside it — 37.1 ms per step against 35.8; on a third, normal-priority
    stream — 36.0: the generator fills what the encoder's launches leave idle, and needs to run beside them for that.)"""
    if depth <= 1:
        y = None
        for _ in range(n):
            yi = step(enc, voc, src, sf0, pool_w, pool_f0, max_batch)
            y = yi if yi is not None else y
        return y
    ys = pipe.run(range(n), lambda _i: step_front(enc, src, sf0, pool_w, pool_f0, max_batch), lambda _i, f: step_back(voc, f))
    return next((y for y in reversed(ys) if y is not None), None)       # strong scaling: this rank's last own conversion


def effective_cores() -> int:
    """CPUs this process may actually use: min(affinity mask, cgroup CPU quota)."""
    n = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    try:
        q, per = open("/sys/fs/cgroup/cpu.max").read().split()
        if q != "max":
            n = min(n, max(1, int(int(q) / int(per))))
    except (OSError, ValueError):
        try:
            q = int(open("/sys/fs/cgroup/cpu/cpu.cfs_quota_us").read())
            per = int(open("/sys/fs/cgroup/cpu/cpu.cfs_period_us").read())
            if q > 0:
                n = min(n, max(1, q // per))
        except (OSError, ValueError):
            pass
    return n


def cpu_baseline(snap):
    """CPU port of the reference path (the oracle) timed stage by stage on bounded samples of THIS step's
    data, scaled to the full step: 1 of 21 WavLM chunks, 300 of 1500 kNN query rows, 150 of 1500 frames of
    each concat re-selection, 25 Adam iterations of each smoothness loop (scaled to the iteration counts the
    device loop needed on the same inputs), 100 of 1500 frames of vocoder.  Every stage: one untimed warm-up
    call (MKL / FFT plan / allocator first-touch — the 0.1 s vs 18 s spread of the `side` stage in round 1 was
    exactly that), then the MEDIAN of three timed calls; fixed thread count = the cgroup's CPU quota.
    ~30-50 s of host work in total."""
    import statistics
    from oracle import knn_ref, select_ref, smooth_ref, synth_ref, vocoder_ref, wavlm_ref
    cores = effective_cores()
    torch.set_num_threads(cores)
    cfg, h = C.WAVLM_LARGE, C.HIFIGAN_V1
    sdw = S.seeded_state(S.wavlm_param_spec(cfg, 6), seed=1)
    sdg = S.seeded_state(S.generator_param_spec(h, "mix"), seed=2)
    t, spread, sampled = {}, {}, [0.0]

    def timed(name, scale, fn, reps=3):
        fn()                                                   # warm-up, untimed
        xs = []
        for _ in range(reps):
            t0 = time.perf_counter(); fn(); xs.append(time.perf_counter() - t0)
        t[name] = statistics.median(xs) * scale
        spread[name] = (min(xs) * scale, max(xs) * scale)
        sampled[0] += sum(xs)                                  # host seconds actually spent in timed calls
    wav = snap["src"]
    timed("wavlm", 21.0, lambda: wavlm_ref.full_features(sdw, cfg, wav, 6))
    # the reference itself runs all 24 layers and keeps layer 6 (ddsp_prematch_dataset.py:289): one more
    # transformer layer on the same [1500, 1, 1024] activations, x 18, is what its --device cpu path pays on top
    x_l = torch.randn(1500, 1, cfg["encoder_embed_dim"], generator=torch.Generator().manual_seed(0))
    pb = wavlm_ref.position_bias(sdw, cfg, 1500)
    with torch.inference_mode():
        timed("wavlm_extra_layer", 21.0 * 18.0, lambda: wavlm_ref.encoder_layer(sdw, cfg, 0, x_l, pb))
    t_extra = t.pop("wavlm_extra_layer"); spread.pop("wavlm_extra_layer")
    timed("side", 21.0, lambda: synth_ref.harmonic_amps(synth_ref.stft_mag(wav)[:1500], snap["qf0"]))
    q, P = snap["q"], snap["P"]
    timed("knn", 5.0, lambda: knn_ref.knn_topk(q[:300], P, 32))
    nn32 = snap["nn32"]
    sh = select_ref.shift_query_f0(snap["qf0"], snap["Pf0"])
    timed("concat_plain", 10.0, lambda: select_ref.concat_reselect(nn32[:150, :4].clone(), q[:150], P, concat_weight=0.2))
    rk = select_ref.rerank_by_f0(sh, snap["Pf0"], nn32)
    timed("concat_f0", 10.0, lambda: select_ref.concat_reselect(rk[:150, :4].clone(), q[:150], P, sh[:150], snap["Pf0"], 0.2))
    it_w, it_h = max(1, snap["iters_wavlm"]), max(1, snap["iters_harm"])
    timed("adam_wavlm", it_w / 25.0, lambda: smooth_ref.smooth_weights(snap["idx_wavlm"], P, 0.1, max_iter=25))
    timed("adam_harm", it_h / 25.0, lambda: smooth_ref.smooth_weights(snap["idx_harm"], snap["Ph"], 1000.0, max_iter=25))
    n = 100
    timed("vocoder", 15.0, lambda: vocoder_ref.synthesizer(sdg, h, "mix", snap["of"][:n][None], snap["s0"][:n][None, :, None],
                                                          snap["hw"][:n][None]))
    total = sum(t.values())
    lo, hi = sum(v[0] for v in spread.values()), sum(v[1] for v in spread.values())
    return dict(value=round(SRC_SECONDS / total, 4), unit="x real-time", cores=cores, kind="port",
                extrapolated=True,          # every stage is timed on a bounded sample and scaled to the full step (see `sample`)
                stage_seconds={k: round(v, 2) for k, v in t.items()}, full_step_seconds=round(total, 1),
                sampled_seconds=round(sampled[0], 1),
                value_range=[round(SRC_SECONDS / hi, 4), round(SRC_SECONDS / lo, 4)],
                reference_equiv_24_layers=round(SRC_SECONDS / (total + t_extra), 4),
                torch_threads=torch.get_num_threads(), timing="1 warm-up + median of 3 per stage",
                sample="oracle stages on this step's data, scaled: 1/21 WavLM chunks (6 layers, the early exit the build "
                       "uses; reference_equiv_24_layers adds 18 x one measured transformer layer per chunk, what the "
                       "reference's own 24-layer call costs), 300/1500 kNN rows, 150/1500 concat "
                       f"frames x2, 25 Adam iterations x2 (scaled to {it_w}/{it_h} device iterations), 100/1500 vocoder frames; "
                       "estimated full-step seconds: " + ", ".join(f"{k} {v:.1f}" for k, v in t.items()) +
                       f", 18 extra WavLM layers {t_extra:.1f}; torch {torch.__version__} CPU")


def other_configs(enc, voc, dev):
    """BASELINE cfg 5 (one GPU's share) and cfg 3 through the PRODUCT entry points, timed by the driver's own run of this
    file (these numbers used to exist only in builder-run tool output).  Rank 0 at N = 1 only, ~20 s.
      cfg5_share: 32 x 30 s sources against a resident 60-minute pool (180 000 frames) through serving.BatchConverter
                  (grouped fused kNN searches, three match lanes, generator tail); sources encoded inside the clock.
      cfg3:       KNeighborsVC.bulk_match over 4 speakers x 80 utterances of 5-10 s, --dur_limit 600 (10-minute pools),
                  files -> files (reads, f0 loads, pool encoding once per file, matching, vocoding, WAV writes in the clock)."""
    import shutil
    import tempfile
    import numpy as np
    from knn_svc_amd import audio_io, matching, serving
    from knn_svc_amd.matcher import KNeighborsVC
    out = {}
    vc = KNeighborsVC(enc, voc, C.HIFIGAN_V1, dev)
    n = 30 * C.SAMPLE_RATE
    with torch.inference_mode():
        t0 = time.perf_counter()
        tv = serving.TargetVoice.from_clips(vc, [S.synth_clip(n, seed=5000 + i) for i in range(120)])
        reqs = [(torch.from_numpy(w).to(dev), torch.from_numpy((f * 1.3).astype(np.float32)).to(dev))
                for w, f in (S.synth_clip(n, seed=7000 + i) for i in range(32))]
        conv = serving.BatchConverter(vc, tv, "mix", "post_opt_0.2")
        conv.convert(reqs); conv.convert(reqs)                 # first sight runs eagerly, the second captures the graphs
        torch.cuda.synchronize()
        setup = time.perf_counter() - t0
        t0 = time.perf_counter()
        reps = 3
        for _ in range(reps):
            ys = conv.convert(reqs)
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t0) / reps
        assert len(ys) == 32 and ys[0].numel() == n
        out["cfg5_share"] = {"workload": "BASELINE cfg 5, one GPU's share: 32 x 30 s sources vs a resident 60-min pool (180 000 frames), mix, "
                                         "post_opt_0.2, through serving.BatchConverter (sources resident in HBM, encoded inside the clock)",
                             "value": round(32 * 30 / dt, 1), "unit": "x real-time", "ms_per_source": round(dt / 32 * 1e3, 2),
                             "knn_pairs_per_s": round(32 * 1500 * tv.frames / dt, 0), "setup_s": round(setup, 1)}
        del tv, conv, reqs, ys
        root = tempfile.mkdtemp(prefix="knnsvc_cfg3_")
        try:
            data = os.path.join(root, "data")
            rng = np.random.default_rng(3)
            secs = 0.0
            for s in range(4):
                d = os.path.join(data, f"spk{s:02d}")
                os.makedirs(d, exist_ok=True)
                for u in range(80):
                    m = int(rng.uniform(5.0, 10.0) * C.SAMPLE_RATE)
                    w, f0 = S.synth_clip(m, 100000 + 1000 * s + u)
                    audio_io.write_wav_pcm16(os.path.join(d, f"u{u:03d}.wav"), w, C.SAMPLE_RATE)
                    np.save(os.path.join(d, f"u{u:03d}_f0.npy"), (f0 * (1.0 + 0.15 * s)).astype(np.float32))
                    secs += m / C.SAMPLE_RATE
            res = []
            for p in range(2):                                  # pass 2: every graph bucket captured (steady state)
                matching._POOL_CACHE = None                     # every pass encodes every file once (cold pool store)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                written = vc.bulk_match(data, data, os.path.join(root, f"out{p}"), ckpt_type="mix", post_opt="post_opt_0.2",
                                        duration_limit=600)
                torch.cuda.synchronize()
                res.append((time.perf_counter() - t0, len(written)))
            matching._POOL_CACHE = None
            out["cfg3"] = {"workload": f"BASELINE cfg 3: bulk_match, 4 speakers x 80 utterances (5-10 s, {secs:.0f} s of audio), every speaker "
                                       "to every other one, dur_limit 600 s, mix, post_opt_0.2, files in -> files out",
                           "value": round(3 * secs / res[1][0], 1), "unit": "x real-time", "first_pass_value": round(3 * secs / res[0][0], 1),
                           "files_written": res[1][1], "wall_s": round(res[1][0], 2)}
        finally:
            shutil.rmtree(root, ignore_errors=True)
    return out


def dump_outputs(out_dir, y, rank):
    """--dump-outputs: what the timed path handed its caller in its last step, the converted waveform (float32, 30 s at 16 kHz),
    as DIR/waveform.npy (rank r > 0: DIR/waveform_rank<r>.npy).  Inputs and weights are seeded, so two builds run with the same
    arguments can be compared output for output.  Copied to the host at once: later passes (--full) replay the same graphs."""
    if y is None:                      # --scaling strong: this rank owned no conversion of the timed steps
        return
    os.makedirs(out_dir, exist_ok=True)
    name = "waveform" if rank == 0 else f"waveform_rank{rank}"
    np.save(os.path.join(out_dir, name + ".npy"), y.detach().float().cpu().numpy())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--max-batch", type=int, default=32, help="30 s chunks per WavLM batch")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: skip the CPU baseline")
    ap.add_argument("--no-other-configs", action="store_true", help="with --full: skip the cfg 3 / cfg 5-share figures (rank 0, N = 1; ~20 s)")
    ap.add_argument("--full", action="store_true",
                    help="also measure everything beyond the headline: latency and long-Adam passes, the eager roofline / kNN pass, "
                         "the CPU baseline and the cfg 3 / cfg 5-share figures")
    ap.add_argument("--dump-outputs", metavar="DIR", help="write the last timed step's waveform to DIR/waveform.npy (float32)")
    ap.add_argument("--stages", action="store_true", help="print per-stage ms to stderr (implies --full)")
    ap.add_argument("--timed-only", action="store_true", help="tracing aid: stop after the timed region (no latency / roofline passes, no JSON line)")
    ap.add_argument("--scaling", choices=("weak", "strong"), default="weak",
                    help="weak (default): one 30 s source + one 10-min pool shard PER RANK (pool and kNN work grow with N); "
                         "strong: ONE 30 s source against ONE 10-min pool whose 20 clips are split over the ranks "
                         "(north_star's pool-shard scaling of a fixed pool; match + vocoder run replicated)")
    ap.add_argument("--pipeline-depth", type=int, default=2, choices=(1, 2),
                    help="2 = overlap match+vocoder of conversion i with the encoder of conversion i+1 (default); 1 = sequential")
    a = ap.parse_args()
    if a.steps < 1:
        ap.error("--steps must be at least 1")
    a.full = a.full or a.stages        # the stage table comes from the eager pass

    ws = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs an MI355X: the product path has no CPU fallback")
    # KNNSVC_BENCH_REHEARSE=1: every rank on cuda:0 under a gloo group (knn_svc_amd.dist then stages the collectives through
    # host memory) — the N > 1 code path run on a ONE-GPU box before the driver runs it on a node.  Its line carries
    # "rehearsal": true and is not a measurement (the ranks share one card).
    rehearse = os.environ.get("KNNSVC_BENCH_REHEARSE") == "1"
    if rehearse:
        local = 0
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    launched = "RANK" in os.environ and "MASTER_ADDR" in os.environ          # started by torch.distributed.run
    if ws > 1 or launched:
        if rehearse:
            dist.init_process_group("gloo")
        else:
            dist.init_process_group("nccl", device_id=dev)
    if a.gpus != ws:
        raise SystemExit(f"bench.py: --gpus {a.gpus} but WORLD_SIZE={ws} (torch.distributed.run --nproc-per-node must equal --gpus)")
    global STRONG
    STRONG = a.scaling == "strong"
    if STRONG and ws > POOL_CLIPS:
        raise SystemExit(f"--scaling strong splits {POOL_CLIPS} pool clips: at most {POOL_CLIPS} ranks")

    # KNNSVC_BENCH_DUMMY_STREAMS=n (A/B aid): n unrelated streams made and used once before anything else — round 4's headline moved by
    # +-8 % with the NUMBER of streams a process had created before (HIP's stream -> hardware-queue mapping: profiles/r04_rank1_rccl_ab.txt);
    # since round 5 the generator needs no streams of its own and the figure must not care (profiles/r05_stream_robustness_ab.txt)
    _dummies = [torch.cuda.Stream(device=dev) for _ in range(int(os.environ.get("KNNSVC_BENCH_DUMMY_STREAMS", "0")))]
    for _s in _dummies:
        with torch.cuda.stream(_s):
            torch.zeros(8, device=dev)
    enc = WavLMEncoder(S.seeded_state(S.wavlm_param_spec(C.WAVLM_LARGE, 6), seed=1), C.WAVLM_LARGE, dev, 6)
    voc = Vocoder(S.seeded_state(S.generator_param_spec(C.HIFIGAN_V1, "mix"), seed=2), C.HIFIGAN_V1, "mix", dev)
    src, sf0, pool_w, pool_f0 = make_inputs(rank, dev)
    timer = GemmTimer()
    if a.full:
        timer.install()
    timer.all_variants = a.stages

    def barrier():
        if dist.is_initialized():
            dist.barrier()
        torch.cuda.synchronize()

    pipe = LanePipeline(dev, lanes=1) if a.pipeline_depth > 1 else None
    args = (enc, voc, src, sf0, pool_w, pool_f0, a.max_batch, pipe)
    with torch.inference_mode():
        for _ in range(2):        # one-time setup outside W: split weights, then hipGraph capture (a shape is captured at its second sight)
            step(enc, voc, src, sf0, pool_w, pool_f0, a.max_batch)
        if a.warmup:
            run_steps(a.warmup, a.pipeline_depth, *args)
        barrier()
        t0 = time.perf_counter()
        y = run_steps(a.steps, a.pipeline_depth, *args)
        barrier()
        dt = time.perf_counter() - t0
        if a.dump_outputs:
            dump_outputs(a.dump_outputs, y, rank)
        if a.timed_only:
            if rank == 0:
                print(f"timed region only: {dt / a.steps * 1e3:.3f} ms/step", file=sys.stderr)
            if dist.is_initialized():
                dist.destroy_process_group()
            return
        if a.full:
            # latency of ONE conversion with nothing overlapped (reported next to the throughput figure)
            t1 = time.perf_counter()
            run_steps(a.steps, 1, *args)
            barrier()
            dt_seq = time.perf_counter() - t1
            # Sensitivity of the headline figure to the length of the two Adam smoothness loops: on these synthetic features
            # they stop at the earliest plateau exit (~200 / ~400 iterations); the reference's cap is 100 000 and real data can
            # run thousands (ddsp_prematch_dataset.py:613-680).  Same pipelined K steps with both loops forced to 2000 iterations.
            ops.ADAM_FORCED_ITERS = LONG_ADAM_ITERS
            run_steps(1, a.pipeline_depth, *args)
            barrier()
            t2 = time.perf_counter()
            run_steps(a.steps, a.pipeline_depth, *args)
            barrier()
            dt_long = time.perf_counter() - t2
            ops.ADAM_FORCED_ITERS = None
            # Roofline pass: the timed region replays hipGraphs (encoder, vocoder), and HIP events cannot be
            # recorded around individual launches inside a replayed graph.  The same K steps are therefore run
            # once more eagerly with an event pair around every launch of the dominant kernel, on its own stream.
            # (only the encoder goes eager: its launches are the ones timed.  The generator keeps replaying its graph — run eagerly,
            #  its ~110 launches on three streams left the HOST behind the GPU, and every timing of the following conversion then
            #  included launch gaps: dominant-kernel fraction 0.47 instead of 0.51, kNN stage 0.86 instead of 0.46 ms)
            # (and the encoder's launch sequence comes from the host in this pass — KNNSVC_WAVLM_HOST_SEQ: since round 5 the product path
            #  enqueues it inside ONE C call, knnsvc_wavlm_encode, where no event can be recorded between two launches; same kernels,
            #  same arguments, same bits: tests/test_gpu_models.py::test_wavlm_one_call_equals_the_host_sequenced_forward)
            enc.use_graphs = False
            os.environ["KNNSVC_WAVLM_HOST_SEQ"] = "1"
            timer.enabled = True
            stage.on = True                     # five event pairs per step; the table is printed only with --stages
            for _ in range(a.steps):
                step(enc, voc, src, sf0, pool_w, pool_f0, a.max_batch)
            barrier()
            timer.enabled = False
            os.environ.pop("KNNSVC_WAVLM_HOST_SEQ", None)
            enc.use_graphs = True
    kdist.raise_if_any_nan()                                            # the deferred NaN flags of every sharded search of this run
    if y is not None:                                                   # strong scaling with fewer steps than ranks: not every rank owned one
        assert y.numel() == SRC_SECONDS * C.SAMPLE_RATE, y.numel()      # 1500 frames x 320
        assert bool(torch.isfinite(y).all()), "non-finite waveform"
    else:
        # strong scaling with fewer timed steps than ranks: not every rank owned a conversion of the last pass — rank 0 included
        # (the owner index runs on from the set-up and warm-up conversions; found by the 5-rank rehearsal of round 5: K = 2)
        assert STRONG
    tmax = torch.tensor([dt], device=dev, dtype=torch.float64)
    if dist.is_initialized():
        if dist.get_backend() == "gloo":
            tmax = tmax.cpu()
        dist.all_reduce(tmax, op=dist.ReduceOp.MAX)
    dt = float(tmax.item())
    fams = timer.summary()
    dom_tags, n_launch, gemm_ms, gemm_flop, dom_floats = fams[0] if fams else (timer.dominant[:1], 0, 0.0, 0.0, 0)
    if a.stages and rank == 0:
        agg = {}
        for e0, e1, fl, shp, var in timer.records:
            t = agg.setdefault((var,) + shp, [0, 0.0, 0.0]); t[0] += 1; t[1] += e0.elapsed_time(e1); t[2] += fl
        for shp, (cnt, ms, fl) in sorted(agg.items(), key=lambda kv: -kv[1][1]):
            print(f"[gemm] {shp[0]:6s} m={shp[1]:7d} n={shp[2]:5d} k={shp[3]:5d} z={shp[4]:3d}  x{cnt // a.steps:3d}/step  {ms / a.steps:8.3f} ms/step  {fl / ms / 1e9:7.1f} TFLOP/s",
                  file=sys.stderr)
        for k, ev in STAGES.items():
            ms = [x.elapsed_time(y_) for x, y_ in ev]
            print(f"[stage] {k:14s} {sum(ms) / max(1, len(ms)):9.3f} ms/step", file=sys.stderr)

    if rank == 0:
        import glob
        ms_step = dt / a.steps * 1e3
        value = (1 if STRONG else ws) * SRC_SECONDS * a.steps / dt      # strong: ONE conversion per step, all ranks on it
        achieved = gemm_flop / (gemm_ms * 1e-3) / 1e12 if gemm_ms > 0 else 0.0
        peak, mfmas, kernel_name = {
            "Q256S": (F16X2_PEAK_TFLOPS, 3, "conv_gemm2quad_kernel<Gemm2QuadS> (implicit GEMM, 256x256 block / 128x128 wave tiles of v_mfma_f32_16x16x32_f16, fp32 emulated as 3 fp16 MFMAs)"),
            "Q256": (F16X2_PEAK_TFLOPS, 3, "conv_gemm2quad_kernel<Gemm2QuadR> (implicit GEMM, 256x256 block / 128x128 wave tiles, fp32 emulated as 3 fp16 MFMAs)"),
            "F128": (F16X2_PEAK_TFLOPS, 3, "conv_gemm2_kernel<Gemm2Tile<128,128,2,2,2,2>> (implicit GEMM, fp32 emulated as 3 fp16 MFMAs)"),
            "H128": (BF16X3_PEAK_TFLOPS, 6, "conv_gemm3_kernel<Gemm3Tile<128,128,2,2,2,2>> (implicit GEMM, fp32 emulated as 6 bf16 MFMAs)"),
            "G128v8": (FP32_MFMA_PEAK_TFLOPS, 1, "conv_gemm_kernel<GemmTile<128,128,2,2,2,2>, 8> (implicit GEMM on v_mfma_f32_32x32x2_f32)"),
        }[dom_tags[0]]
        line = {
            "metric": "audio-sec converted/sec (xRT) end-to-end, cold target pool",
            "value": round(value, 3), "unit": "x real-time", "n_gpus": ws, "steps": a.steps, "warmup": a.warmup,
            "ms_per_step": round(ms_step, 3), "higher_is_better": True, "scaling": a.scaling, "vs_baseline": None,
            "dtype": "f32", "data": "synthetic",
            **({"rehearsal": True, "rehearsal_note": f"all {ws} ranks share cuda:0 under gloo with host-staged collectives: exercises the "
                "N > 1 code path, NOT a measurement"} if os.environ.get("KNNSVC_BENCH_REHEARSE") == "1" else {}),
            "config": {"workload": ("north-star point, ONE conversion per step: 30 s source vs ONE 10 min target pool (20 x 30 s) "
                                    f"split over the {ws} rank(s), " if STRONG else
                                    "north-star point per rank: 30 s source vs 10 min target pool (20 x 30 s), ") +
                                   "ckpt_type=mix, post_opt_0.2, cold (pool encoded inside the step); seeded random "
                                   "weights of WavLM-Large (6 layers executed) and the 22.9 M-param generator",
                       "nq": 1500, "np_per_rank": (30000 // ws if STRONG else 30000),
                       "pool_sharding": (f"one pool, rows over {ws} rank(s) in file order, replicated queries, RCCL all-gather merge of the top-32 lists; "
                                         f"match + generator of conversion i on rank i mod {ws} only, pool rows to that rank point-to-point"
                                         if STRONG else ("none: one rank searches its whole 30 000-row pool (no process group, no collective)" if ws == 1 else
                                                         f"weak: every rank holds its own 30 000-row shard and searches all {ws} x 1500 query frames in it; "
                                                         "top-32 lists exchanged with one RCCL all-to-all and merged (lower index first on ties)")),
                       "wavlm_batch_chunks": a.max_batch,
                       "pipeline_depth": a.pipeline_depth,
                       "pipeline": ("match + vocoder of conversion i run on a second stream under the encoder of conversion i+1; the pipeline's "
                                    "streams are chosen by measured contention (pipeline.new_stream), not by creation order"
                                    if a.pipeline_depth > 1 else "none: conversions run one after the other")},
        }
        line["config"]["adam_iterations"] = [int(step.last["iters_wavlm"]), int(step.last["iters_harm"])]
        if a.full:
            line["config"]["sequential_ms_per_step"] = round(dt_seq / a.steps * 1e3, 3)
            line["roofline"] = {"bound": "mfma", "achieved": round(achieved, 2), "peak": round(peak, 1), "unit": "TFLOP/s",
                                "frac": round(achieved / peak, 4), "traffic": None,
                                "kernel": kernel_name,
                                "note": f"achieved = algorithmic fp32 FLOP (2*M*N*K per launch) / HIP-event time; peak = dense 16-bit "
                                        f"MFMA peak 2500 TFLOP/s / {mfmas} MFMAs per product; executed MFMA rate = {mfmas} x achieved",
                                "frac_of_fp32_mfma_peak_157.3": round(achieved / FP32_MFMA_PEAK_TFLOPS, 4),
                                "timing": "HIP events around each launch in an eager, host-sequenced re-run of the same K steps right after the "
                                          "timed region (which replays hipGraphs of the one-call encoder)",
                                "launches": n_launch, "avg_launch_ms": round(gemm_ms / max(1, n_launch), 4),
                                "kernel_ms_per_step": round(gemm_ms / a.steps, 3),
                                "secondary": [{"kernel": "+".join(f), "launches": nl, "kernel_ms_per_step": round(ms / a.steps, 3),
                                               "achieved": round(fl / (ms * 1e-3) / 1e12, 2) if ms > 0 else 0.0,
                                               "frac": round(fl / (ms * 1e-3) / 1e12 / peak, 4) if ms > 0 else 0.0}
                                              for f, nl, ms, fl, _b in fams[1:]]}
            tl = torch.tensor([dt_long], device=dev, dtype=torch.float64)
            line["value_long_adam"] = {"value": round((1 if STRONG else ws) * SRC_SECONDS * a.steps / float(tl.item()), 3),
                                       "adam_iterations": [LONG_ADAM_ITERS, LONG_ADAM_ITERS],
                                       "ms_per_step": round(float(tl.item()) / a.steps * 1e3, 3),
                                       "note": "same pipelined steps with both smoothness loops forced to 2000 iterations (stopping rules "
                                               "off): the headline value's sensitivity to data on which the loops run long; rank 0's clock"}
        # BASELINE.json's second metric: kNN query frames/s and its roofline (MFMA-bound once Nq >= ~64).
        # One kNN stage = every rank's 1500 query frames against the whole pool (each rank searches all ws*1500 queries in
        # its own 30 000-row shard: row norms, f16x2 split of the shard and the queries, q.p^T GEMM, distance formula +
        # top-32, then the all-gather merge).  HIP events around the stage in the eager pass, rank 0's stream.
        if STAGES.get("knn"):
            kms = [x.elapsed_time(y_) for x, y_ in STAGES["knn"]]
            kms = sum(kms) / len(kms)
            nq_all, np_shard, D = (1500, 1500 * -(-POOL_CLIPS // ws), 1024) if STRONG else (ws * 1500, 30000, 1024)
            flop = 2.0 * nq_all * np_shard * D                     # per rank
            tfl = flop / (kms * 1e-3) / 1e12
            min_bytes = 4.0 * D * (nq_all + np_shard) + 8 * 32 * nq_all
            line["knn"] = {"query_frames_per_s": round(nq_all / (kms * 1e-3), 0), "ms": round(kms, 4),
                           "nq_per_rank": 1500, "nq_searched_per_rank": nq_all, "np_shard": np_shard, "np_total": (30000 if STRONG else ws * np_shard), "k": 32,
                           "tflops_fp32_equiv_per_gpu": round(tfl, 1),
                           "bound": "mfma", "frac_f16x2_ceiling_833": round(tfl / F16X2_PEAK_TFLOPS, 4),
                           "frac_fp32_mfma_peak_157.3": round(tfl / FP32_MFMA_PEAK_TFLOPS, 4),
                           "t_mfma_floor_ms": round(flop / (F16X2_PEAK_TFLOPS * 1e12) * 1e3, 4),
                           "t_hbm_floor_ms": round(min_bytes / 8e12 * 1e3, 4),
                           "route": "fused (epochs of knn_screen + knn_refine on the Gemm2QuadS loop: no [Nq, Np] distance or dot matrix in HBM), then "
                                    "knn_rescore: the listed pairs re-scored from exact (fp64-accumulated) dot products",
                           "note": "whole stage incl. row norms, operand splits, both epochs' screening GEMMs, top-32 refinement, the exact re-score, and the "
                                   "RCCL list exchange + merge; query_frames_per_s counts every rank's frames resolved against the whole pool"}
        # counted (not inferred) MFMA utilisation of the search's kernels: rocprofv3 --pmc SQ_VALU_MFMA_BUSY_CYCLES / GRBM_GUI_ACTIVE over
        # the same search size (tools/pmc_knn.sh -> profiles/rNN_pmc_knn.json; bench.py cannot read PMCs itself)
        if "knn" in line:
            for pmc in sorted(glob.glob(os.path.join(ROOT, "profiles", "r*_pmc_knn.json")), reverse=True):
                t = json.load(open(pmc))
                if t.get("nq") == 1500 and t.get("np") == 30000 and "screen_mfma_util" in t:
                    line["knn"]["mfma_util_counted"] = {"knn_screen_kernel": round(t["screen_mfma_util"], 4), "whole_search": round(t["search_mfma_util"], 4),
                                                        "source": f"profiles/{os.path.basename(pmc)}: SQ_VALU_MFMA_BUSY_CYCLES / (1024 SIMDs x GRBM_GUI_ACTIVE / 8), "
                                                                  "one rocprofv3 --pmc pass over tools/knn_prof_one.py 1500 30000"}
                    break
        # measured offline with rocprofv3 --pmc (tools/pmc_traffic.py, tools/refresh_profiles.sh); bench.py cannot read PMCs itself.
        # Newest round's file whose kernel is the one reported above.
        if a.full:
            want = {"Q256S": "Gemm2QuadS", "Q256": "Gemm2QuadR"}.get(dom_tags[0], "Gemm2Tile<128, 128" if dom_tags[0].startswith("F128") else None)
            for pmc in sorted(glob.glob(os.path.join(ROOT, "profiles", "r*_pmc_traffic.json")), reverse=True):
                t = json.load(open(pmc))
                if want and want in t.get("kernel", ""):
                    line["roofline"]["traffic"] = t["hbm_bytes_per_launch"]
                    line["roofline"]["traffic_source"] = (f"profiles/{os.path.basename(pmc)}: 2*FETCH_SIZE + WRITE_SIZE per launch, "
                                                          "separate rocprofv3 --pmc passes")
                    line["roofline"]["algorithmic_bytes_per_launch"] = int(4 * dom_floats / max(1, n_launch))
                    break
        if a.full and ws == 1 and not a.no_cpu_baseline:
            L = step.last
            c = lambda x: x.detach().cpu()
            snap = dict(src=c(src), q=c(L["q"]), qf0=c(L["qf0"]), P=c(L["P"]), Pf0=c(L["Pf0"]), Ph=c(L["Ph"]), nn32=c(L["nn32"]),
                        idx_wavlm=c(L["idx_wavlm"]), idx_harm=c(L["idx_harm"]), of=c(L["of"]), hw=c(L["hw"]), s0=c(L["s0"]),
                        iters_wavlm=int(L["iters_wavlm"]), iters_harm=int(L["iters_harm"]))
            line["cpu_baseline"] = cpu_baseline(snap)
        if a.full and ws == 1 and not a.no_other_configs and not a.stages:
            import contextlib
            with contextlib.redirect_stdout(sys.stderr):        # bulk_match prints its progress like the reference: keep stdout ONE line
                line["other_configs"] = other_configs(enc, voc, dev)
        print(json.dumps(line), flush=True)
    if dist.is_initialized():
        dist.destroy_process_group()


if __name__ == "__main__":
    try:
        main()
    except ops.KnnOverflow:
        # a row of some search had more than 4096 survivors in one epoch (thousands of bit-identical pool rows inside the first epoch:
        # adversarial data, never seen on the synthetic clips): the searches of this run are void.  Once more, on the dot-matrix route.
        print("bench.py: fused kNN route overflowed its candidate buffer; re-running on the dot-matrix route", file=sys.stderr)
        if dist.is_initialized():
            dist.destroy_process_group()
        os.environ["KNNSVC_KNN_FUSED"] = "0"
        main()
