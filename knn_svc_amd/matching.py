"""Feature-pool building and frame matching on the GPU.

Host-side mirror of the reference's ``get_complete_spk_pool`` and
``match_at_inference_time`` (ddsp_prematch_dataset.py:301-414, 1074-1459): same
arguments, same returned dict-of-tensors keyed by ``str(path)``, same quirks
(k hard-coded to 32 -> first 4, ``--dur_limit`` in seconds overshooting by one file,
``post_opt`` parsing, ``prioritize_f0`` must be True, pool rebuilt per call).
``topk``, ``vad_trigger_level`` (accepted and dropped upstream), ``f0_shift``, ``transpose`` and ``tune`` are extension knobs:
knn_svc_amd/options.py has the tables; ``resolve_topk`` / ``resolve_f0_shift`` / ``resolve_dynamics`` / ``resolve_tune`` below are
their checks.
All arithmetic is done by libknnsvc_hip.so kernels on device-resident tensors; the
only host work is file I/O and the chunk bookkeeping.
"""
from __future__ import annotations

import contextlib
import math
import os
import types
from pathlib import Path

import numpy as np
import torch

from . import audio_io, config as C, dist as kdist, features, ops, pipeline, pool_cache
from .options import TUNE_OFF, Extensions, Harmony, HarmonyShift, SourceKnobs, Tuning, per_item
from .wavlm import WavLMEncoder, chunk_plan

AUDIO_EXT = {".flac", ".wav", ".mp3"}


def parse_post_opt(post_opt: str):
    """(concat_weight, run_adam): float of the last '_' token, 'extra' -> 0.3, else -1 (off);
    the Adam stage is skipped iff 'no_post_opt' is a substring (ddsp_prematch_dataset.py:1273-1279, 1356)."""
    tail = post_opt.split("_")[-1]
    try:
        w = float(tail)
    except ValueError:
        w = 0.3 if tail == "extra" else -1
    return w, ("no_post_opt" not in post_opt)


def list_audio(path) -> list:
    """A single audio file, or every audio file under a folder in sorted rglob order (:313-319)."""
    path = Path(path)
    if os.path.isfile(path) and os.path.splitext(path)[-1] in AUDIO_EXT:
        files = [path]
    else:
        files = sorted([p for p in path.rglob("**/*") if p.suffix.lower() in AUDIO_EXT])
        assert len(files) != 0, [f"directory not containing any audio {path}"]
    # The reference decodes every listed container through torchaudio (:332).  Here .wav and .flac are decoded natively and
    # .mp3 only when soundfile is importable: a pool that holds a file nobody can decode is refused NOW, by name, not in the
    # middle of a run after the other files have been encoded.
    bad = [str(p) for p in files if not audio_io.can_decode(p.suffix)]
    if bad:
        raise RuntimeError(f"{len(bad)} audio file(s) under {path} are in a container this build cannot decode without the "
                           f"'soundfile' package (.wav and .flac are native): {bad[:5]}{' ...' if len(bad) > 5 else ''} — "
                           "transcode them to .wav / .flac or install soundfile")
    return files


def load_utterance(pth):
    """-> (wav float32 [L] mono 16 kHz on the host, f0 float32 array).  Channel mean for multi-channel
    input (:333-335); f0 from ``<stem>_f0.npy`` (:373-382)."""
    x, sr = audio_io.load_audio(str(pth))
    if x.shape[0] > 1:
        x = x.mean(axis=0, keepdims=True)
    if sr != C.SAMPLE_RATE:      # on the GPU (features.resample); the reference resamples with torchaudio on the host (:338-341)
        x = features.resample(torch.from_numpy(np.ascontiguousarray(x[0], dtype=np.float32)).cuda(), sr,
                              C.SAMPLE_RATE).cpu().numpy()[None]
    f0_path = os.path.splitext(str(pth))[0] + "_f0.npy"
    if not os.path.isfile(f0_path):
        # same bookkeeping as the reference (:376-379): warn, compute, write the cache next to the audio.  The reference runs
        # pyworld.harvest on the host here (:121-128); this build runs Harvest on the GPU (csrc/harvest.hip, fp64, pinned on
        # the reference's own shipped tracks).
        xg = torch.from_numpy(np.ascontiguousarray(x[0], dtype=np.float32)).cuda()
        print(f"WARNING: {f0_path} not exists, generating...")
        f0_new = ops.f0_harvest(xg).cpu().numpy()
        np.save(f0_path, f0_new)
    f0 = np.asarray(np.load(f0_path, allow_pickle=True), dtype=np.float32)
    return np.ascontiguousarray(x[0], dtype=np.float32), f0


def frames_of(n_samples: int, enc: WavLMEncoder) -> int:
    return sum(enc.n_frames(l + p) for (_s, l, p) in chunk_plan(n_samples))


def side_features(wav_gpu: torch.Tensor, f0_host: np.ndarray, T: int):
    """STFT magnitude -> harmonic amplitudes for one utterance (:361-404).  Returns (f0 [T], harm [T,49], spec [T,200])."""
    assert wav_gpu.numel() >= C.HOP * T
    spec = features.stft_mag(wav_gpu)
    assert spec.shape[0] >= T
    spec = spec[:T].contiguous()
    assert abs(len(f0_host) - T) <= 1 and len(f0_host) >= T, [len(f0_host), T]
    if isinstance(f0_host, torch.Tensor):           # already resident on the device
        f0 = f0_host[:T].contiguous()
    else:
        f0 = torch.from_numpy(np.ascontiguousarray(f0_host[:T])).to(wav_gpu.device)
    harm = ops.harmonic_amps(spec, f0, C.N_HARM)
    return f0, harm, spec


def side_features_many(wavs_gpu, f0s_host, Ts):
    """``side_features`` for a list of utterances in four launches (features.stft_harm_batch) instead of four per file.
    -> list of (f0 [T], harm [T,49], spec [T,200]); identical values."""
    if wavs_gpu and not wavs_gpu[0].is_cuda:          # (CPU tensors: the gloo tests inject their stand-in at ``side_features``)
        return [side_features(w, f0, T) for w, f0, T in zip(wavs_gpu, f0s_host, Ts)]
    f0s = []
    for w, f0, T in zip(wavs_gpu, f0s_host, Ts):
        assert w.numel() >= C.HOP * T
        assert abs(len(f0) - T) <= 1 and len(f0) >= T, [len(f0), T]
        f0s.append(f0[:T].contiguous() if isinstance(f0, torch.Tensor)
                   else torch.from_numpy(np.ascontiguousarray(f0[:T])).to(w.device, non_blocking=True))
    res = features.stft_harm_batch(wavs_gpu, f0s, Ts, n_harm=C.N_HARM)
    return [(f0, harm, spec) for f0, (spec, harm) in zip(f0s, res)]


VAD_MIN_LEVEL = 1e-3          # trimming is active above this trigger level (upstream's test, ddsp_matcher.py:462)


def vad_active(vad_trigger_level) -> bool:
    return vad_trigger_level is not None and vad_trigger_level > VAD_MIN_LEVEL


def vad_tag(vad_trigger_level) -> tuple:
    """What the trimming adds to a pool-store key: nothing when it is off (existing keys do not move)."""
    return (("vad", float(vad_trigger_level)),) if vad_active(vad_trigger_level) else ()


def disk_identity(wavlm, vad_trigger_level=0) -> tuple:
    """What an on-disk pool-store entry belongs to besides its audio file: the encoder's WEIGHTS, its exit layer and the layer
    weighting the features were mixed under (set_layer_mix bumps ``uid`` for the in-memory tier; the disk tier outlives the
    process, so it needs the weighting itself — without it a second weighting read back the first one's features), and the
    trigger level the file was trimmed with, when it was."""
    return (wavlm.weights_fingerprint(), wavlm.n_layers, getattr(wavlm, "layer_mix", None)) + vad_tag(vad_trigger_level)


def slice_f0(f0, lstrip: int, T: int):
    """The f0 track of a recording trimmed by ``lstrip`` samples in front (a multiple of the hop) and ``T`` frames long: the
    track is computed and cached on the UNTRIMMED file (``<stem>_f0.npy`` stays valid) and cut here; T or T + 1 values."""
    assert lstrip % C.HOP == 0, lstrip
    a = lstrip // C.HOP
    return f0[a:a + T + 1]


def trim_silence(w, f0, vad_trigger_level, wavlm):
    """One loaded utterance (host arrays) with the silence at both ends removed (ops.vad_trim on the encoder's device) ->
    (wav, f0) of the kept range, or None when the trimmer finds no speech in it."""
    strip = ops.vad_trim(torch.from_numpy(w).to(wavlm.device), vad_trigger_level, C.SAMPLE_RATE)
    lstrip, rstrip = (int(v) for v in strip[0].cpu())
    if lstrip < 0:
        return None
    w = np.ascontiguousarray(w[lstrip:len(w) - rstrip])
    return w, slice_f0(f0, lstrip, frames_of(len(w), wavlm))


def get_complete_spk_pool(path, wavlm: WavLMEncoder, match_weights=None, synth_weights=None, device="cuda",
                          duration_limit=None, vad_trigger_level=0, shard_files=False, gather=False):
    """Per-file dicts (matching_pool, synth_pool, audio_synth_pool, spec_synth_pool, f0_pool, harmonics_pool),
    like the reference.  matching == synth features under the encoder's CURRENT layer mix (both weightings are the same one-hot on
    the live path; match_at_inference_time calls this once per weighting when they differ);
    ``audio_synth_pool`` is kept as None values: the live path never reads it (audio_out_feats_weighted = None,
    ddsp_prematch_dataset.py:1368).  Per-file results are kept in the device-resident pool store
    (knn_svc_amd/pool_cache.py) so that dataset mode encodes every file once instead of once per speaker pair.
    ``shard_files`` (one process per GPU): every rank walks the same file list and duration limit, but encodes and
    returns only its contiguous share of the kept files (dist.contiguous_share) — the pool shard of BASELINE cfg 4.
    ``gather`` (with shard_files): the shares are all-gathered afterwards (features and f0 only — what a QUERY pool
    needs), so every rank returns the complete per-file dicts although it encoded only its share.
    ``vad_trigger_level`` > 1e-3 (upstream's threshold; an extension — upstream's function never reads the argument): every
    file is trimmed of the silence at both ends right after it is loaded (``trim_silence``: the restated sox `vad`, parity with
    torchaudio unpinned); its frame count, features, spectrum and harmonics come from the trimmed waveform, its f0 from the
    track of the untrimmed file cut to match.  A file without speech is skipped with a printed line, a pool without any file
    left is an error.  Every rank trims every file it lists, so the kept files and their lengths agree across ranks."""
    dev = wavlm.device
    files = list_audio(path)
    cache = _pool_cache()
    vad = vad_active(vad_trigger_level)
    tag = (wavlm.uid, wavlm.n_layers) + vad_tag(vad_trigger_level)
    dtag = disk_identity(wavlm, vad_trigger_level) if cache.disk_dir else None     # on-disk tier: content identity
    dkeys = {}
    kept, keys, Ts = [], [], []
    loaded = {}                       # index -> (wav host, f0 host) for files that miss the cache
    hits = {}                         # index -> cache entry: held here, a later put() may evict it from the store
    dur = 0.0
    for pth in files:
        i = len(kept)
        key = pool_cache.file_key(pth, tag)
        if dtag is not None:
            dkeys[key] = pool_cache.file_key(pth, dtag)
        ent = cache.get(key, dkeys.get(key), dev)
        if ent is not None:
            T = ent["feats"].shape[0]
            hits[i] = ent
        else:
            w, f0 = load_utterance(pth)
            key = pool_cache.file_key(pth, tag)                   # load_utterance may have just written <stem>_f0.npy,
            if dtag is not None:                                  # which is part of the file's identity
                dkeys[key] = pool_cache.file_key(pth, dtag)
            if vad:
                cut = trim_silence(w, f0, vad_trigger_level, wavlm)
                if cut is None:
                    print(f"VAD trimming {pth} {vad_trigger_level}: no speech found, file skipped")
                    continue
                w, f0 = cut
            T = frames_of(len(w), wavlm)
            loaded[i] = (w, f0)                                   # host arrays: only this rank's share goes to the device
        kept.append(str(pth)); keys.append(key); Ts.append(T)
        dur += T * C.HOP / C.SAMPLE_RATE
        if duration_limit is not None and dur >= duration_limit:
            break
    if not kept:
        raise ops.KnnSvcError(f"VAD trimming at level {vad_trigger_level} left no file of {path} in the pool")
    lo, hi = kdist.contiguous_share(len(kept)) if shard_files else (0, len(kept))
    loaded = {i: (torch.from_numpy(v[0]).to(dev), v[1]) for i, v in loaded.items() if lo <= i < hi}
    miss = sorted(loaded)
    feats = wavlm.encode_many([loaded[i][0] for i in miss], pow2_batches=True) if miss else []
    sides = side_features_many([loaded[i][0] for i in miss], [loaded[i][1] for i in miss], [Ts[i] for i in miss])
    for i, ft, (f0, harm, spec) in zip(miss, feats, sides):
        assert ft.shape[0] == Ts[i]
        hits[i] = dict(feats=ft, f0=f0, harm=harm, spec=spec)
        cache.put(keys[i], hits[i], dkeys.get(keys[i]))
    matching, synth, audio, specs, f0p, harmp = {}, {}, {}, {}, {}, {}
    if shard_files and gather and kdist.world()[1] > 1:
        # query pool: every rank needs every file's features and f0 (replicated kNN queries); rank order = file order
        mine = [hits[i] for i in range(lo, hi)]
        E = wavlm.E
        cat = lambda k, shape: (torch.cat([e[k] for e in mine], 0).contiguous() if mine
                                else torch.empty(shape, device=dev, dtype=torch.float32))
        counts = kdist.shard_rows(sum(Ts[lo:hi]), dev)
        all_f = kdist.all_gather_rows_var(cat("feats", (0, E)), counts)
        all_f0 = kdist.all_gather_rows_var(cat("f0", (0,)), counts)
        r0 = 0
        for key, T in zip(kept, Ts):
            matching[key] = synth[key] = all_f[r0:r0 + T]
            f0p[key] = all_f0[r0:r0 + T]
            audio[key] = specs[key] = harmp[key] = None
            r0 += T
        return matching, synth, audio, specs, f0p, harmp
    for i, key in enumerate(kept):
        if not lo <= i < hi:
            continue
        ent = hits[i]
        matching[key] = ent["feats"]; synth[key] = ent["feats"]; audio[key] = None
        specs[key] = ent["spec"]; f0p[key] = ent["f0"]; harmp[key] = ent["harm"]
    return matching, synth, audio, specs, f0p, harmp


_POOL_CACHE = None


def _pool_cache():
    global _POOL_CACHE
    if _POOL_CACHE is None:
        _POOL_CACHE = pool_cache.PoolCache()
    return _POOL_CACHE


_SIDE = {}


def _side_stream(device) -> "torch.cuda.Stream":
    """Partner stream of the CURRENT stream (one per (device, stream)): concurrent match_features calls on
    different streams (pipeline.LanePipeline) must not meet on one shared side stream."""
    idx = torch.device(device).index if torch.device(device).index is not None else torch.cuda.current_device()
    key = (idx, torch.cuda.current_stream(idx).cuda_stream)
    if key not in _SIDE:
        from .pipeline import new_stream
        cur = torch.cuda.current_stream(idx)
        # a partner has to run BESIDE its stream — and beside the lanes, tails and other partners: measured at creation
        # (pipeline.new_stream, overlap_with="all"), not left to the stream -> hardware-queue mapping
        from . import pipeline
        vetted = [st for (d_, _k, _i, _p), st in pipeline._VETTED.items() if d_ == idx]
        if cur.cuda_stream == 0 or any(cur.cuda_stream == st.cuda_stream for st in vetted):
            # the partner of the default stream or of a measured (single-lane) pipeline stream: measured too
            _SIDE[key] = new_stream(idx, priority=cur.priority, kind="partner", overlap_with="all", must=[cur] + vetted)
        else:
            _SIDE[key] = new_stream(idx, priority=cur.priority, kind="partner")
    return _SIDE[key]


def prepare_pool(matching_list, split=True):
    """Per-pool quantities that do not depend on the query (row norms, the split image the kNN GEMM reads): computed
    once per target pool in dataset mode instead of once per utterance.  ``split=False``: norms only (the neighbours
    come from the pool-sharded search)."""
    P = matching_list
    stats = ops.row_norms(P)
    return dict(stats=stats, split=ops.prepare_knn_pool(P, C.KNN_K, stats) if split else None)


# query frames per grouped search in dataset mode.  Measured (tools/knn_group_ab.sh; cfg 5 share, xRT): 1500 -> 2321, 3000 -> 2349,
# 8192 -> 1884, everything in one search -> 1864; cfg 3 is flat (1331-1351).  Groups large enough for the fused screen + refine route
# (>= 4096 rows) LOSE inside a pipeline: its one-block-per-CU, 128 KB-LDS launches leave no room next to them for the single-workgroup
# recurrences and the generator of the other items.  3000 frames keeps the searches on the 128x128 kernel and ahead of the lanes.
KNN_GROUP_FRAMES = int(os.environ.get("KNNSVC_KNN_GROUP_FRAMES", "3000"))
_KNN_STREAMS = {}


def _knn_stream(device) -> "torch.cuda.Stream":
    """The stream the grouped kNN searches of dataset mode run on (ahead of the lanes that consume their results)."""
    key = torch.device(device).index if torch.device(device).index is not None else torch.cuda.current_device()
    if key not in _KNN_STREAMS:
        from .pipeline import new_stream
        _KNN_STREAMS[key] = new_stream(device, kind="knn")
    return _KNN_STREAMS[key]


# CUs a grouped search's screening kernel may occupy inside the dataset-mode pipeline (it is persistent: a block walks tiles); the
# rest stays free for the single-workgroup recurrences and the generator of the items in flight.  0 = all.
KNN_PIPE_BLOCKS = int(os.environ.get("KNNSVC_KNN_PIPE_BLOCKS", "192"))


def batched_knn(q_all, matching_list, prep, max_blocks=0):
    """Top-32 of the stacked frames of many query utterances against one prepared pool -> (idx [sum Nq, 32], flag: NaN /
    overflow bits, read by the caller at the end)."""
    idx, _d, fl = ops.knn_topk(q_all, matching_list, C.KNN_K, p_stats=prep["stats"], prepared=prep["split"],
                               check_nan=False, return_flag=True, max_blocks=max_blocks)
    return idx, fl


def grouped_knn(items, query_pool, matching_list, prep, flags):
    """Top-32 of every item's frames against one prepared pool, searched in GROUPS of at least KNN_GROUP_FRAMES query frames
    one after the other on a stream of their own: group g + 1 is searched while the match bodies and the generator of group g
    run, instead of one search of everything in front of the whole pipeline (32 x 30 s sources against a 60-minute pool:
    16.1 -> 12.8 ms per source).  -> (nn: item -> [Nq, 32] indices, ready: item -> event a consumer
    on another stream has to wait for; empty without a kNN stream).  Results do not depend on the grouping."""
    nn, nn_ready = {}, {}
    groups, cur_g, cur_n = [], [], 0
    for it in items:
        cur_g.append(it); cur_n += query_pool[it].shape[0]
        if cur_n >= KNN_GROUP_FRAMES:
            groups.append(cur_g); cur_g, cur_n = [], 0
    if cur_g:
        groups.append(cur_g)
    main = torch.cuda.current_stream(matching_list.device) if matching_list.is_cuda else None
    ks = _knn_stream(matching_list.device) if main is not None and len(groups) > 1 else None
    if ks is not None:
        ks.wait_stream(main)
    prod = ks if ks is not None else main          # the stream the searches are enqueued on (None: CPU stand-ins in the gloo tests)
    for grp in groups:
        ctx = torch.cuda.stream(ks) if ks is not None else contextlib.nullcontext()
        with ctx:
            q_all = torch.cat([query_pool[it] for it in grp], 0).contiguous()
            idx_all, fl = batched_knn(q_all, matching_list, prep, max_blocks=KNN_PIPE_BLOCKS if len(groups) > 1 else 0)
            parts = [t.contiguous() for t in idx_all.split([query_pool[it].shape[0] for it in grp])]
            # ALWAYS an ordering token, also for a single group searched on the caller's own stream: the lists are consumed on
            # lane streams, and a tensor handed out without one is a race waiting for a caller that does not happen to wait
            ev = prod.record_event() if prod is not None else None
        if fl is not None:
            flags.append(fl)
        for it, t in zip(grp, parts):
            nn[it] = t
            if ev is not None:
                nn_ready[it] = ev
    return nn, nn_ready


def ordering_token(device):
    """Event on the current stream: the token for neighbour lists produced on it (pool-sharded searches)."""
    return torch.cuda.current_stream(device).record_event()


def wait_for_neighbours(nn_item, ready_event, device):
    """Make the current stream wait for a neighbour list produced on another stream.  Every device-resident list comes with
    the event of its producing stream (grouped_knn, ordering_token); a list without one is refused rather than read early."""
    if nn_item is None:
        return
    if ready_event is None:
        if nn_item.is_cuda:
            raise RuntimeError("wait_for_neighbours: device-resident neighbour list without an ordering event")
        return
    st = torch.cuda.current_stream(device)
    st.wait_event(ready_event)
    nn_item.record_stream(st)


def resolve_topk(topk) -> int:
    """Neighbours mixed per frame: None = C.KNN_USE (4, what the released checkpoints were trained on), else 1..8."""
    if topk is None:
        return C.KNN_USE
    if isinstance(topk, bool) or int(topk) != topk or not 1 <= int(topk) <= 8:
        raise ValueError(f"topk must be an integer in 1..8 (or None for {C.KNN_USE}), got {topk!r}")
    return int(topk)


# How the source's f0 is moved towards the target's (an extension; upstream knows only "median").  The values are the library's
# KNNSVC_F0_SHIFT_* codes; include/knnsvc_hip.h ("Pitch control") is the specification.
#   median    by median(log f0 pool) - median(log f0 source): an arbitrary real interval (upstream, the default)
#   octave    that difference rounded to whole octaves: the pitch classes are kept, the register moves to the target's
#   semitone  that difference rounded to whole semitones: the result stays on the source's equal-tempered grid
#   none      no shift: the medians are not read
# ``transpose`` (semitones, finite, |t| <= F0_TRANSPOSE_MAX) is added on top in every mode.
F0_SHIFT_MODES = {"median": ops.F0_SHIFT_MEDIAN, "octave": ops.F0_SHIFT_OCTAVE, "semitone": ops.F0_SHIFT_SEMITONE,
                  "none": ops.F0_SHIFT_NONE}
F0_TRANSPOSE_MAX = 36.0


def _one_f0_shift(mode, transpose):
    if mode is None:
        mode = "median"
    if not isinstance(mode, str) or mode not in F0_SHIFT_MODES:
        raise ValueError(f"f0_shift must be one of {tuple(F0_SHIFT_MODES)} (or None for 'median'), got {mode!r}")
    if transpose is None:
        transpose = 0.0
    if isinstance(transpose, (bool, np.bool_)) or not isinstance(transpose, (int, float, np.integer, np.floating)):
        raise ValueError(f"transpose must be a number of semitones, got {transpose!r}")
    t = float(np.float32(transpose))                  # the value the library sees
    if not np.isfinite(t) or abs(t) > F0_TRANSPOSE_MAX:
        raise ValueError(f"transpose must be finite and within +-{F0_TRANSPOSE_MAX:g} semitones, got {transpose!r}")
    return F0_SHIFT_MODES[mode], t


def resolve_f0_shift(mode, transpose, n_items=None):
    """``f0_shift`` / ``transpose`` as the library takes them, refused before any device work when they are not valid.
    ``n_items`` None: one mode name (None = "median") and one number (None = 0) -> (code, float).  ``n_items`` = the number of
    items of a batch: each may also be a list / tuple with one entry per item -> (list of codes, list of floats)."""
    if n_items is None:
        if isinstance(mode, (list, tuple)) or isinstance(transpose, (list, tuple)):
            raise ValueError("f0_shift / transpose: a single value expected here, not a list")
        return _one_f0_shift(mode, transpose)
    pairs = [_one_f0_shift(m, t) for m, t in zip(per_item(mode, n_items, "f0_shift"), per_item(transpose, n_items, "transpose"))]
    return [m for m, _ in pairs], [t for _, t in pairs]


# ``target_duration`` (seconds; upstream's name, documented there and never delivered: ddsp_matcher.py:524-548 stretches the query
# features only, then exits): the QUERY sequence — features and f0 — is re-timed right behind the encoder (ops.time_scale_seg;
# include/knnsvc_hip.h "Time scale" is the specification), so every stage of the match sees the stretched sequence and the generator
# emits T_out * hop samples.  A duration belongs to a source item, not to the options.Extensions record.
DURATION_SCALE_MIN, DURATION_SCALE_MAX = 0.25, 4.0      # product bound on T_out / T: beyond it the pool's frames are repeated or
                                                        # skipped further than the neighbour smoothing can hide


def _one_target_duration(value):
    if value is None:
        return None
    if isinstance(value, (bool, np.bool_)) or not isinstance(value, (int, float, np.integer, np.floating)):
        raise ValueError(f"target_duration must be a number of seconds (or None for off), got {value!r}")
    d = float(value)
    if not np.isfinite(d) or d <= 0:
        raise ValueError(f"target_duration must be finite and > 0 seconds (or None for off), got {value!r}")
    return d


def resolve_target_duration(value, n_items=None):
    """``target_duration`` checked, refused before any device or file work when it is not valid.  ``n_items`` None: one number
    of seconds, finite and > 0, or None (off) -> float or None.  ``n_items`` = the number of items of a batch: the value may
    also be a list / tuple with one entry per item (None entries: off) -> list of n_items entries."""
    if n_items is None:
        if isinstance(value, (list, tuple)):
            raise ValueError("target_duration: a single value expected here, not a list")
        return _one_target_duration(value)
    return per_item(value, n_items, "target_duration", _one_target_duration)


def duration_plan(T, target_duration, sr=C.SAMPLE_RATE, hop=C.HOP, item=None):
    """-> (T_out, inv_scale) for a query of ``T`` frames and a ``target_duration`` in seconds: upstream's arithmetic verbatim
    (ddsp_matcher.py:546-548), T_out as F.interpolate computes it from its scale factor.  ValueError (naming ``item``) when the
    result has no frame or the scale factor lies outside [DURATION_SCALE_MIN, DURATION_SCALE_MAX]."""
    who = "" if item is None else f" for {item}"
    if int(T) < 1:
        raise ValueError(f"target_duration{who}: the source has no frame")
    target_samples = int(target_duration * sr)
    s = (target_samples / hop) / T
    T_out = int(math.floor(float(T) * s))
    if T_out < 1:
        raise ValueError(f"target_duration{who}: {target_duration!r} s is shorter than one frame ({hop} samples at {sr} Hz)")
    if not DURATION_SCALE_MIN <= s <= DURATION_SCALE_MAX:
        raise ValueError(f"target_duration{who}: {target_duration!r} s for a source of {T} frames ({T * hop / sr:g} s) is a time scale "
                         f"of {s:g}, outside [{DURATION_SCALE_MIN:g}, {DURATION_SCALE_MAX:g}]")
    return T_out, 1.0 / s


def refuse_duration_with_envelope(durations, ext):
    """The envelope mix aligns the source waveform with the output sample for sample, so it cannot be combined with a re-timed
    query (re-timing that envelope is left for later): ValueError when any of ``durations`` is set and ``ext.envelope_mix`` > 0."""
    if ext.envelope_mix > 0 and any(d is not None for d in durations):
        raise ValueError("target_duration cannot be combined with envelope_mix > 0: the envelope stage aligns the source waveform "
                         "with the output sample for sample")


def stretch_queries(feats, f0s, durations):
    """The queries of a batch re-timed to their ``durations`` (seconds, None: left alone): ONE ops.time_scale_seg over the
    stacked items that have one -> (feats', f0s'), per-item views of its outputs; the other items pass through as the very
    same tensors, and without any duration nothing is launched."""
    who = [i for i, d in enumerate(durations) if d is not None]
    if not who:
        return feats, f0s
    plans = [duration_plan(feats[i].shape[0], durations[i], item=f"item {i}") for i in who]
    xo, fo = ops.time_scale_seg(_stacked([feats[i] for i in who]), _stacked([f0s[i] for i in who]),
                                ops.Segments.of_lengths(feats[i].shape[0] for i in who), [p[0] for p in plans], [p[1] for p in plans])
    feats, f0s = list(feats), list(f0s)
    o = 0
    for i, (T_out, _c) in zip(who, plans):
        feats[i], f0s[i] = xo[o:o + T_out], fo[o:o + T_out]
        o += T_out
    return feats, f0s


# Voice blend (an extension; include/knnsvc_hip.h "Voice blend" is the specification): a conversion towards a weighted mix of 2 to
# BLEND_MAX_VOICES target voices.  Each voice is matched as if it were the only target, the matched features and harmonics are
# mixed (ops.blend_seg), and the source's f0 is shifted ONCE, towards the weighted mean of the voices' log-f0 medians
# (ops.shift_f0_seg_blend).  A weight vector belongs to a source item, like a request's own ``transpose``: it is a field of
# options.SourceKnobs, not of options.Extensions.  The library does not normalise; ``resolve_blend`` does, in fp64.
BLEND_MAX_VOICES = ops.BLEND_MAX_VOICES


def _one_blend(value, n_voices):
    if value is None:
        return (1.0 / n_voices,) * n_voices
    if isinstance(value, (str, bytes)) or not isinstance(value, (list, tuple, np.ndarray)):
        raise ValueError(f"blend must be a sequence of {n_voices} weights (or None for equal weights), got {value!r}")
    if len(value) != n_voices:
        raise ValueError(f"blend: {len(value)} weights for {n_voices} voices")
    a = []
    for w in value:
        if isinstance(w, (bool, np.bool_)) or not isinstance(w, (int, float, np.integer, np.floating)):
            raise ValueError(f"blend: a weight must be a number, got {w!r}")
        w = float(w)
        if not math.isfinite(w) or w < 0:
            raise ValueError(f"blend: a weight must be finite and >= 0, got {w!r}")
        a.append(w + 0.0)                              # (-0.0 becomes 0.0)
    try:
        total = math.fsum(a)
    except OverflowError:
        total = math.inf
    if not total > 0 or not math.isfinite(total):
        raise ValueError(f"blend: at least one weight must be > 0 and their sum finite, got {value!r}")
    return tuple(w / total for w in a)


def blend_per_item(weights) -> bool:
    """Whether ``weights`` is a list with one entry per item (vectors or Nones; the empty list too), not one weight vector."""
    return isinstance(weights, (list, tuple)) and (len(weights) == 0 or
                                                   any(w is None or isinstance(w, (list, tuple, np.ndarray)) for w in weights))


def resolve_blend(weights, n_voices, n_items=None):
    """Blend weights as the library takes them, refused (ValueError) before any device or file work when they are not valid:
    ``n_voices`` numbers, finite and >= 0, at least one > 0 (None: equal weights), normalised in fp64 as ``a / math.fsum(a)``
    — a one-hot vector stays exactly one-hot.  ``n_items`` None: one vector -> a tuple.  ``n_items`` = the number of items of a
    batch: one vector for all items, or a list / tuple with one entry per item (a vector, or None for equal weights)
    -> a list of n_items tuples.  ``n_voices`` outside 2..BLEND_MAX_VOICES is refused as well."""
    if isinstance(n_voices, bool) or int(n_voices) != n_voices or not 2 <= int(n_voices) <= BLEND_MAX_VOICES:
        raise ValueError(f"a blend takes 2..{BLEND_MAX_VOICES} voices, got {n_voices!r}")
    n_voices = int(n_voices)
    if n_items is None:
        return _one_blend(weights, n_voices)
    one = lambda w: _one_blend(w, n_voices)
    return per_item(weights, n_items, "blend", one, default=one(None), is_list=blend_per_item, unit="weight vectors")


def refuse_blend_when_sharded():
    """A blend matches every voice's whole pool on one GPU: under KNNSVC_POOL_SHARD=1 (pool rows sharded over the ranks) it is
    refused, before a file is read."""
    if os.environ.get("KNNSVC_POOL_SHARD") == "1":
        raise ValueError("a voice blend cannot be combined with KNNSVC_POOL_SHARD=1 (the pools of a blend are not sharded)")


# Pitch correction (an extension; include/knnsvc_hip.h "Pitch correction" is the specification): the SHIFTED f0 of an item snapped
# towards the notes of a key (ops.tune_f0_seg), right behind the f0 shift and in front of the f0 re-rank, so that the neighbour
# selection, the pitched re-selection and the vocoder all see the corrected contour.  The key is the key of the OUTPUT: correction
# follows the shift, ``transpose``, a blend's one shift and ``target_duration``'s re-timing (``retune_ms`` runs in output time).  With
# "median" the interval is an arbitrary real number and correction is what puts the result on a grid; with "semitone" / "octave" /
# "none" plus a whole ``transpose`` the output's key is the source's key moved by that interval.  A key belongs to a song, that is,
# to a source item: a field of options.SourceKnobs, not of options.Extensions.
def _one_tune(value):
    if value is None or isinstance(value, Tuning):        # (a Tuning is checked when it is built)
        return value
    if isinstance(value, str):
        return TUNE_OFF if value.strip().lower() == "off" else Tuning(scale=value)
    raise ValueError(f"tune must be an options.Tuning, a scale such as 'chromatic' or 'A:minor', 'off' or None, got {value!r}")


def resolve_tune(value, n_items=None):
    """``tune`` checked, refused (ValueError) before any file or device work when it is not valid.  None -> None (nothing of its
    own: the converter's default, or off); "off" -> options.TUNE_OFF, an explicit off for that item; any other string ->
    ``Tuning(scale=...)`` with the default strength, retune time and tuning frequency; a ``Tuning`` -> itself.  ``n_items`` None:
    one value.  ``n_items`` = the number of items of a batch: one value for all items or a list / tuple with one entry per item
    -> a list of n_items entries."""
    if n_items is None:
        if isinstance(value, (list, tuple)):
            raise ValueError("tune: a single value expected here, not a list")
        return _one_tune(value)
    return per_item(value, n_items, "tune", _one_tune)


def tune_active(tunings) -> bool:
    """Whether any entry of a resolved ``tune`` list asks for a correction (an entry that is None or off does not)."""
    return any(t is not None and t.on for t in tunings)


# Harmony voices (an extension; include/knnsvc_hip.h "Harmony voice" is the specification): a source item sung in 1 + P parts by the
# same target voice.  A part is a further ITEM of the match stage whose f0 is the lead's final f0 (shifted and, when on, corrected)
# moved by scale degrees (ops.harmony_f0_seg), right behind ops.tune_f0_seg and in front of the f0 re-rank, so that a part's pool
# frames are the ones sung at the part's pitch.  The parts share the lead's encoder output and neighbour lists (``nn32s``); the
# converter mixes their waveforms (ops.mix_waves).  The match stage takes, per item, the part's options.HarmonyShift or None; the
# user's options.Harmony is resolved by the converter, which knows the item's ``tune``.
HARMONY_OFF = "off"           # what resolve_harmony returns for "off": an item under a converter whose default is on


def _one_harmony(value):
    if value is None or isinstance(value, Harmony):       # (a Harmony is checked when it is built)
        return value
    if isinstance(value, str) and value.strip().lower() == "off":
        return HARMONY_OFF
    raise ValueError(f"harmony must be an options.Harmony, 'off' or None, got {value!r}")


def resolve_harmony(value, n_items=None):
    """``harmony`` checked, refused (ValueError) before any file or device work when it is not valid.  None -> None (nothing of
    its own: the converter's default, or off); "off" -> HARMONY_OFF, an explicit off for that item; an options.Harmony ->
    itself.  ``n_items`` None: one value.  ``n_items`` = the number of items of a batch: one value for all items or a list /
    tuple with one entry per item -> a list of n_items entries."""
    if n_items is None:
        if isinstance(value, (list, tuple)):
            raise ValueError("harmony: a single value expected here, not a list")
        return _one_harmony(value)
    return per_item(value, n_items, "harmony", _one_harmony)


def harmony_of(value, tune=None):
    """A resolved ``harmony`` entry and the item's resolved ``tune`` -> (the options.Harmony, its HarmonyShift per part), or None
    when the item has no harmony.  ValueError when neither names a scale."""
    if value is None or value == HARMONY_OFF:
        return None
    return value, value.shifts(tune)


def _one_shift(value):
    if value is None or isinstance(value, HarmonyShift):
        return value
    raise ValueError(f"harmony: the match stage takes an options.HarmonyShift per item (Harmony.shifts) or None, got {value!r}")


def resolve_harmony_shifts(value, n_items):
    """The match stage's ``harmony`` argument: one options.HarmonyShift (or None) for all items, or a list with one per item
    -> a list of n_items entries."""
    return per_item(value, n_items, "harmony", _one_shift)


def harmony_active(shifts) -> bool:
    """Whether any entry of a resolved list of part records moves its item (None or an off record does not)."""
    return any(p is not None and p.on for p in shifts)


def resolve_dynamics(envelope_mix, peak_db):
    """The two output-dynamics switches as the library takes them, refused before any device or file work when they are not
    valid -> (a, p).  ``envelope_mix``: a number in [0, 1], None = 0 (off): how much of the source's volume envelope the tail
    puts back on the generated waveform (ops.envelope_mix).  ``peak_db``: None (off) or a finite number <= 0: the sample-peak
    ceiling in dBFS the tail holds the waveform under (ops.limit_peak)."""
    num = lambda v: not isinstance(v, (bool, np.bool_)) and isinstance(v, (int, float, np.integer, np.floating))
    a = 0.0 if envelope_mix is None else envelope_mix
    if not num(a) or not 0.0 <= float(a) <= 1.0:                      # (NaN compares false)
        raise ValueError(f"envelope_mix must be a number in [0, 1] (or None for 0 = off), got {envelope_mix!r}")
    if peak_db is not None and (not num(peak_db) or not np.isfinite(float(peak_db)) or float(peak_db) > 0.0):
        raise ValueError(f"peak_db must be a finite number of dBFS <= 0 (or None for no ceiling), got {peak_db!r}")
    return float(a), None if peak_db is None else float(peak_db)


def match_features(query_seq, query_f0, matching_list, matching_f0, harmonics_list, ckpt_type, post_opt,
                   return_debug=False, nn32=None, nan_flags=None, pool_prep=None, synth_list=None, topk=None,
                   f0_shift=None, transpose=None, tune=None, harmony=None):
    """The per-query body (ddsp_prematch_dataset.py:1189-1450) on device tensors: ``match_features_many`` (below, where the
    arguments are described) of one utterance.  ``nn32`` may carry neighbours already found by the pool-sharded search
    (knn_svc_amd.dist.sharded_knn); in the debug dict ``iters_*`` are one-element tensors, or 0 without the Adam stage."""
    resolve_f0_shift(f0_shift, transpose)     # one value each
    resolve_tune(tune)
    part = {} if harmony is None else dict(harmony=[_one_shift(harmony)])
    return match_features_many([query_seq], [query_f0], matching_list, matching_f0, harmonics_list, ckpt_type, post_opt,
                               nn32s=None if nn32 is None else [nn32], nan_flags=nan_flags, pool_prep=pool_prep,
                               synth_list=synth_list, return_debug=return_debug, topk=topk, f0_shift=f0_shift,
                               transpose=transpose, tune=tune, **part)[0]


# How the match stage of SEVERAL items is put on the chip: "lanes" (one match_features per item on the lane streams, the default) or
# "segmented" (match_features_many: the items of a batch stacked, one workgroup per item in every recurrence launch).
MATCH_MODES = ("lanes", "segmented")
# Items per segmented batch.  16 is a GUESS (a quarter of the 64 segments one launch takes; enough items for the kNN groups to stay
# ahead of the batches) until tools/match_seg_ab.py has been run on the hardware: its sweep row for 32 x 30 s sources replaces it.
MATCH_BATCH_DEFAULT = 16


def match_mode(match=None) -> str:
    """The route: the argument, else KNNSVC_MATCH, else "lanes"."""
    m = match if match is not None else (os.environ.get("KNNSVC_MATCH") or "lanes")
    if m not in MATCH_MODES:
        raise ValueError(f"match must be one of {MATCH_MODES}, got {m!r}")
    return m


def match_batch_size(match_batch=None) -> int:
    """Items per segmented batch: the argument, else KNNSVC_MATCH_BATCH, else MATCH_BATCH_DEFAULT."""
    n = int(match_batch if match_batch is not None else (os.environ.get("KNNSVC_MATCH_BATCH") or MATCH_BATCH_DEFAULT))
    if n < 1:
        raise ValueError("match_batch must be >= 1")
    return n


def _stacked(ts):
    """The tensors' rows one after the other (a single tensor as it is)."""
    return ts[0].contiguous() if len(ts) == 1 else torch.cat([t.contiguous() for t in ts], 0).contiguous()


def _split(t, lens):
    """The stacked rows of ``t`` per item again (views); None: a None per item."""
    return t.split(lens) if t is not None else [None] * len(lens)


def match_features_many(query_seqs, query_f0s, matching_list, matching_f0, harmonics_list, ckpt_type, post_opt, nn32s=None,
                        nan_flags=None, pool_prep=None, synth_list=None, return_debug=False, topk=None, f0_shift=None,
                        transpose=None, tune=None, harmony=None):
    """The per-query body (ddsp_prematch_dataset.py:1189-1450) for several query utterances against one pool, run ONCE over their
    stacked frames -> a list of per-item tuples (out_feats, harm or None, shifted_f0[, debug dict]) (views of the stacked outputs).
    The row-wise stages (row norms, f0 re-rank, weighted sums) take the stacked rows as they are; the per-sequence stages (median,
    shift, concat re-selection, smoothness weights) take the segment table: one workgroup per item, so item i's tensors are
    bit-identical to the call with item i alone and the same ``nn32``.  ``synth_list``: the pool under the SYNTHESIS layer weighting
    when it differs from the matching one (:349-350, 1157): the search and the concat re-selection run on ``matching_list``, the
    smoothness weights and the weighted sums on ``synth_list`` (:1260, 1347-1350).  ``nn32s``: per-item neighbour lists (or None: one
    search over the stacked frames).  ``nan_flags``: a list that receives the kNN NaN flag instead of the host checking it here
    (the caller then calls ``ops.raise_if_nan`` on each entry once everything is enqueued — keeps a stream pipeline free of syncs).
    ``topk``: neighbours kept per frame out of the 32 found (1..8; None = 4, the specialised kernels).
    ``f0_shift`` / ``transpose``: how each item's f0 is moved (F0_SHIFT_MODES; a value for all items or a list with one per item;
    None = "median" / 0).  The interval is chosen per item on the device (ops.shift_f0_seg with modes): no host read of the
    medians; the defaults are the same call with the median / 0 tables.  The debug dict carries ``shift_semitones``: the interval
    applied to the item (a one-element device tensor).
    ``tune``: the pitch correction of each item (``resolve_tune``'s argument: a value for all items or one per item; None / "off":
    none).  When any item has one, the shifted f0 goes through ops.tune_f0_seg right behind the shift, on the side stream, so the
    re-rank, the pitched concat re-selection and the returned f0 (the vocoder's) all see the corrected contour; otherwise nothing
    is launched.  The debug dict carries ``tuned_notes``: the item's int32 note per frame (-1: not corrected), None when off;
    ``shift_semitones`` stays the shift's interval.
    ``harmony``: per item the options.HarmonyShift of a harmony part (``resolve_harmony_shifts``: one for all items or one per
    item; None: the item is a lead).  When any item has one, the shifted (and corrected) f0 goes through ops.harmony_f0_seg right
    behind the correction, on the side stream: re-rank, pitched re-selection and the returned f0 see the part's contour;
    otherwise nothing is launched.  The debug dict carries ``harmony_notes``: the part's int32 note per frame, None when off."""
    topk = resolve_topk(topk)                 # before any device work
    shift_modes, shift_ts = resolve_f0_shift(f0_shift, transpose, len(query_seqs))
    tunings = resolve_tune(tune, len(query_seqs))
    parts = resolve_harmony_shifts(harmony, len(query_seqs))
    lens = [int(q.shape[0]) for q in query_seqs]
    seg = ops.Segments.of_lengths(lens)       # the host tables once for the six segmented calls
    q = _stacked(query_seqs)
    query_f0 = _stacked([t.reshape(-1) for t in query_f0s])
    P = matching_list
    qn, qs = ops.row_norms(q)
    pn, ps = pool_prep["stats"] if pool_prep is not None else ops.row_norms(P)
    nan_flag = None
    if nn32s is None or any(t is None for t in nn32s):
        # NaN check deferred to the end of the launch sequence (one host sync instead of a split stream)
        nn32, _, nan_flag = ops.knn_topk(q, P, C.KNN_K, q_stats=(qn, qs), p_stats=(pn, ps), check_nan=False,
                                         return_flag=True, prepared=pool_prep["split"] if pool_prep is not None else None)
    else:
        nn32 = _stacked(list(nn32s))
    cw, run_adam = parse_post_opt(post_opt)
    with_harm = "wavlm_only" not in ckpt_type and "no_harm_no_amp" not in ckpt_type
    # The WavLM-feature branch (concat re-selection -> Adam -> weighted sum) and the pitched branch
    # (f0 shift -> re-rank -> concat re-selection -> Adam on harmonics) only share nn32, and each is a
    # chain of single-workgroup latency-bound kernels: run them on two HIP streams.
    main = torch.cuda.current_stream()
    side = _side_stream(q.device)
    side.wait_stream(main)
    it1 = it2 = None
    w = w2 = harm_w = None
    with torch.cuda.stream(side):
        qmed, pmed = ops.log_f0_median_seg(query_f0, seg), ops.log_f0_median(matching_f0)      # the pool's median once
        shifted = ops.shift_f0_seg(query_f0, seg, qmed, pmed, shift_modes, shift_ts, return_shift=return_debug)
        shifted, semis = shifted if return_debug else (shifted, None)
        notes = None
        if tune_active(tunings):
            shifted = ops.tune_f0_seg(shifted, seg, tunings, return_notes=return_debug)
            shifted, notes = shifted if return_debug else (shifted, None)
        hnotes = None
        if harmony_active(parts):
            shifted = ops.harmony_f0_seg(shifted, seg, parts, return_notes=return_debug)
            shifted, hnotes = shifted if return_debug else (shifted, None)
        ranked = ops.f0_rerank(nn32, shifted, matching_f0)
        idx2 = ranked[:, :topk].contiguous()
        if cw != -1:
            idx2 = ops.concat_reselect_seg(idx2, seg, q, qn, P, pn, shifted, matching_f0, concat_weight=cw)
        if with_harm:
            if run_adam:
                w2, it2 = ops.smooth_weights_seg(idx2, seg, harmonics_list, 1000.0, return_iters=True)
            harm_w = ops.weighted_gather(idx2, w2, harmonics_list, mean=True)        # without Adam: torch.mean (:1446)
    idx = nn32[:, :topk].contiguous()
    if cw != -1:
        idx = ops.concat_reselect_seg(idx, seg, q, qn, P, pn, concat_weight=cw)
    Ps = synth_list if synth_list is not None else P
    if run_adam:
        w, it1 = ops.smooth_weights_seg(idx, seg, Ps, 0.1, return_iters=True)
    out_feats = ops.weighted_gather(idx, w, Ps)                                      # without Adam: softmax(ones) (:1361-1364)
    main.wait_stream(side)
    for t in (shifted, semis, notes, hnotes, idx2, harm_w, w2, it2):
        if t is not None:
            t.record_stream(main)
    if nan_flag is not None:
        if nan_flags is not None:
            nan_flags.append(nan_flag)
        else:
            try:
                ops.raise_if_nan(nan_flag)
            except ops.KnnOverflow:         # the fused route's candidate buffer overflowed: once more on the dot-matrix route
                with ops.fused_off():
                    return match_features_many(query_seqs, query_f0s, matching_list, matching_f0, harmonics_list, ckpt_type, post_opt,
                                               pool_prep=pool_prep, synth_list=synth_list, return_debug=return_debug, topk=topk,
                                               f0_shift=f0_shift, transpose=transpose, tune=tune, harmony=harmony)
    out = []
    dbg = [_split(t, lens) for t in (nn32, idx, w, idx2, w2, notes, hnotes)]
    for i, (of, hw, sf) in enumerate(zip(_split(out_feats, lens), _split(harm_w, lens), _split(shifted, lens))):
        if return_debug:
            out.append((of, hw, sf, dict(nn32=dbg[0][i], idx_wavlm=dbg[1][i], w_wavlm=dbg[2][i], idx_harm=dbg[3][i], w_harm=dbg[4][i],
                                         iters_wavlm=it1[i:i + 1] if it1 is not None else 0,
                                         iters_harm=it2[i:i + 1] if it2 is not None else 0,
                                         shift_semitones=semis[i:i + 1], tuned_notes=dbg[5][i], harmony_notes=dbg[6][i])))
        else:
            out.append((of, hw, sf))
    return out


def match_features_blend(query_seqs, query_f0s, voices, weights, ckpt_type, post_opt, nn32s=None, nan_flags=None, topk=None,
                         f0_shift=None, transpose=None, tune=None, harmony=None):
    """``match_features_many`` towards a weighted mix of 2..BLEND_MAX_VOICES ``voices`` (serving.TargetVoice, or anything with
    ``feats`` / ``f0`` / ``harm`` and optionally ``prep`` / ``synth``: ``match_bodies``) -> the same list of
    per-item tuples (out_feats, harm or None, shifted_f0).  ``weights``: ``resolve_blend``'s argument (one vector for all items or
    one per item; None: equal).  One ``match_features_many`` per voice — its pool, f0, harmonics, ``pool_prep``, ``synth_list``
    and the items' own ``f0_shift`` / ``transpose`` / ``topk``, so every voice's frames are bit-identical to the single-target
    conversion towards it —, then ONE ops.blend_seg for the features and one for the harmonics (none when the checkpoint type has
    no harmonics), then ONE ops.shift_f0_seg_blend: the returned f0 is the source's, shifted once towards the weighted mean of the
    voices' log medians (the per-voice shifted tracks are used inside each voice's match only).  A voice whose weight is 0 for
    every item is not matched.  ``nn32s``: per voice, the per-item neighbour lists of ``match_features_many`` (or None).  NaN
    flags and the overflow retry work per voice, as there.  ``tune``: as there, inside every voice's match (each on that voice's
    shifted track) and, through one more ops.tune_f0_seg, on the returned f0: the blend's one shift, corrected.  ``harmony``: as
    there too: inside every voice's match and once more, behind that correction, on the returned f0."""
    rows = resolve_blend(weights, len(voices), len(query_seqs))      # before any device work
    resolve_topk(topk)
    tunings = resolve_tune(tune, len(query_seqs))
    tuned = dict(tune=tunings) if tune_active(tunings) else {}
    parts = resolve_harmony_shifts(harmony, len(query_seqs))
    if harmony_active(parts):
        tuned["harmony"] = parts
    shift_modes, shift_ts = resolve_f0_shift(f0_shift, transpose, len(query_seqs))
    live = [v for v in range(len(voices)) if any(r[v] != 0.0 for r in rows)]
    per = {}
    for v in live:
        vo = voices[v]
        per[v] = match_features_many(query_seqs, query_f0s, vo.feats, vo.f0, vo.harm, ckpt_type, post_opt,
                                     nn32s=None if nn32s is None else nn32s[v], nan_flags=nan_flags, pool_prep=getattr(vo, "prep", None),
                                     synth_list=getattr(vo, "synth", None), topk=topk, f0_shift=f0_shift, transpose=transpose, **tuned)
    lens = [int(q.shape[0]) for q in query_seqs]
    seg = ops.Segments.of_lengths(lens)
    # a voice that was not matched has weight 0 in every row: its pointer is never read, any live voice's stands in
    def stacked(k):
        got = {v: _stacked([r[k] for r in per[v]]) for v in live}
        return [got.get(v, got[live[0]]) for v in range(len(voices))]
    out_feats = ops.blend_seg(stacked(0), seg, rows)
    with_harm = per[live[0]][0][1] is not None
    harm = ops.blend_seg(stacked(1), seg, rows) if with_harm else None
    query_f0 = _stacked([t.reshape(-1) for t in query_f0s])
    qmed = ops.log_f0_median_seg(query_f0, seg)
    meds = {v: ops.log_f0_median(voices[v].f0) for v in live}
    pmeds = torch.stack([meds.get(v, meds[live[0]]) for v in range(len(voices))]).contiguous()
    shifted = ops.shift_f0_seg_blend(query_f0, seg, qmed, pmeds, rows, shift_modes, shift_ts)
    if "tune" in tuned:
        shifted = ops.tune_f0_seg(shifted, seg, tunings)
    if "harmony" in tuned:
        shifted = ops.harmony_f0_seg(shifted, seg, parts)
    return list(zip(_split(out_feats, lens), _split(harm, lens), _split(shifted, lens)))


def match_bodies(query_of, voices, ckpt_type, post_opt, found, flags, knobs, topk=None, parts=None):
    """-> the ``(body, body_many)`` pair of ``run_match_bodies``: the match of one item, and of a batch of items stacked.
    ``query_of(item)`` -> (features, f0) of the item's query.  ``voices``: a list of one voice (serving.TargetVoice, or anything
    with ``feats`` / ``f0`` / ``harm`` and optionally ``prep`` / ``synth``), or of 2..BLEND_MAX_VOICES for a blend
    (``match_features_blend``, on both routes).  ``found``: per voice, ``(nn: item -> neighbour list, ready: item -> event)`` of the
    searches already enqueued (``grouped_knn``); an item not in ``nn`` is searched inside its match.  ``flags``: receives the
    deferred NaN flags.  ``knobs(item)`` -> the item's options.SourceKnobs: its ``f0_shift`` / ``transpose`` and, for a blend, its
    weight row, and its ``tune`` (handed on only when an item of the batch has one that is on: without it the match functions are
    called as they always were).  ``parts(item)`` -> the options.HarmonyShift of an item that is a harmony part, or None (a record
    of its own beside the knobs); ``parts`` None: no item is one.  Handed on by the same rule as ``tune``."""
    dev = voices[0].feats.device

    def match(batch, alone):
        for nn, ready in found:
            for i in batch:
                wait_for_neighbours(nn.get(i), ready.get(i), dev)      # a group search on the kNN stream
        nn32s = [[nn.get(i) for i in batch] for nn, _ready in found]
        qs, f0s = (list(t) for t in zip(*(query_of(i) for i in batch)))
        ks = [knobs(i) for i in batch]
        modes, semis = [k.f0_shift for k in ks], [k.transpose for k in ks]
        tunes = [k.tune for k in ks]
        tuned = tune_active(tunes)
        moves = [None] * len(batch) if parts is None else [parts(i) for i in batch]
        part = harmony_active(moves)
        if len(voices) > 1:
            return match_features_blend(qs, f0s, voices, [k.blend for k in ks], ckpt_type, post_opt, nn32s=nn32s, nan_flags=flags,
                                        topk=topk, f0_shift=modes, transpose=semis, **(dict(tune=tunes) if tuned else {}),
                                        **(dict(harmony=moves) if part else {}))
        vo = voices[0]
        pool = dict(nan_flags=flags, pool_prep=getattr(vo, "prep", None), synth_list=getattr(vo, "synth", None), topk=topk)
        if alone:              # (through the module global: the CPU tests put their stand-in there)
            return [match_features(qs[0], f0s[0], vo.feats, vo.f0, vo.harm, ckpt_type, post_opt, nn32=nn32s[0][0], f0_shift=modes[0],
                                   transpose=semis[0], **(dict(tune=tunes[0]) if tuned else {}),
                                   **(dict(harmony=moves[0]) if part else {}), **pool)]
        return match_features_many(qs, f0s, vo.feats, vo.f0, vo.harm, ckpt_type, post_opt, nn32s=nn32s[0], f0_shift=modes,
                                   transpose=semis, **(dict(tune=tunes) if tuned else {}), **(dict(harmony=moves) if part else {}), **pool)
    return (lambda item: match([item], True)[0]), (lambda batch: match(batch, False))


def run_match_bodies(items, body, body_many, tail=None, *, device, lanes, match="lanes", match_batch=None):
    """The match bodies of ``items``, and ``tail(item, result)`` behind each, on the lane / tail streams of a pipeline.LanePipeline
    -> the results in item order.  ``match`` "lanes": ``body(item)`` per item; "segmented" (several items): the items in order, in
    batches of ``match_batch``, each batch one ``body_many(batch)`` on a lane.  What a tail needs besides the match result (the
    item's source waveform, for the envelope mix) it finds by ``item``: the callers' tails close over it.  CPU tensors (the injected kernels of the gloo tests)
    and a single lane without a tail run on the caller's stream, one after the other."""
    items = list(items)
    dev = torch.device(device)
    segmented = match == "segmented" and len(items) > 1 and dev.type == "cuda"
    if not items or dev.type != "cuda" or (tail is None and lanes <= 1 and not segmented):
        heads = (body(i) for i in items)
        return [h if tail is None else tail(i, h) for i, h in zip(items, heads)]
    pipe = pipeline.LanePipeline(dev, max(1, lanes))
    if segmented:
        nb = match_batch_size(match_batch)
        return pipe.run_batched([items[a:a + nb] for a in range(0, len(items), nb)], body_many, tail)
    return pipe.run(items, body, tail)


def vocoding_tail(vocode_fn, items, source_of):
    """The ``tail(item, result)`` of ``run_match_bodies`` around a ``vocode_fn(out_feats, shifted_f0, harm)`` -> the item's
    waveform.  A ``vocode_fn`` whose ``needs_source`` attribute is true (matcher.Tail with the envelope mix)
    also gets ``src_wav=source_of(item)``, the item's waveform as the encoder received it, on the device: all of them are fetched
    here, before the pipeline starts, since the tail only enqueues.  Any other callable is called with the three arguments."""
    if not getattr(vocode_fn, "needs_source", False):
        return lambda item, r: vocode_fn(r[0], r[2], r[1])
    src = {it: source_of(it) for it in items}
    return lambda item, r: vocode_fn(r[0], r[2], r[1], src_wav=src[item])


def _mix_of(weights, wavlm):
    """A layer weighting as the encoder takes it: None for the one-hot on its exit layer (the live path), else the tuple."""
    if weights is None:
        return None
    w = [float(v) for v in torch.as_tensor(weights).reshape(-1).float().cpu().tolist()]
    if any(v != 0.0 for v in w[wavlm.n_layers + 1:]):
        raise NotImplementedError(f"layer weighting uses layers beyond the {wavlm.n_layers} the encoder was loaded with "
                                  "(load it with n_layers = the last weighted layer)")
    w = (w + [0.0] * (wavlm.n_layers + 1))[:wavlm.n_layers + 1]
    if sum(1 for v in w if v != 0.0) == 1 and w[wavlm.n_layers] == 1.0:
        return None
    return tuple(w)


def match_at_inference_time(src_wav_file, ref_wav_file, wavlm: WavLMEncoder, match_weights=None, synth_weights=None,
                            topk: int = 4, device="cuda", prioritize_f0=False, ckpt_type="wavlm_only",
                            src_dataset_path=None, tgt_dataset_path=None, cache_dir=None, required_subset=None,
                            post_opt="no_post_opt", duration_limit=None, vocode_fn=None, waves_out=None,
                            pool_sharded=None, share_items=False, use_topk=False, use_vad=False, vad_trigger_level=7,
                            f0_shift="median", transpose=0.0, ext=None, target_duration=None, tune=None):
    """Same contract as the reference function (ddsp_prematch_dataset.py:1074).  ``cache_dir`` is ignored (the reference
    force-disables it, :1086-1087).  ``topk`` (k = 32 -> 4 is hard-coded upstream, :1203,1246,1398) / ``use_topk``,
    ``vad_trigger_level`` (upstream passes 7 for the target pool, :1131, to a function that drops it) / ``use_vad``, ``f0_shift``
    and ``transpose`` are the extension knobs of options.Extensions.from_reference, on every route below; ``ext``: that record
    already built by the caller (``special_match``, ``bulk_match``), the six arguments are then not read.  ``target_duration``
    (seconds, None: off; single source file only — with ``src_dataset_path`` a value is refused): the source's features and f0
    are re-timed to that length right behind the encoder (``stretch_queries``), in front of everything of the match stage, so
    the returned tensors have ``duration_plan``'s T_out frames; not to be combined with ``envelope_mix`` > 0.
    ``tune`` (``resolve_tune``: an options.Tuning, a scale, "off" or None; one value): every source item's shifted f0 is snapped
    towards that key inside its match (``match_features_many``); the returned f0 is the corrected one.

    Build extension (BASELINE cfg 5, many sources against one pool): ``vocode_fn(out_feats, shifted_f0, harm)`` is
    enqueued as the pipeline's tail stage right behind each item's match body and its waveform stored in
    ``waves_out[item]`` — the generator of item i then runs underneath the kNN / recurrences of items i+1.., instead
    of after all of them.  It must not synchronise with the host.  A ``vocode_fn`` with a true ``needs_source`` attribute
    (matcher.Tail with the envelope mix) also receives ``src_wav=``, the item's source waveform (``vocoding_tail``); a plain
    three-argument callable loads nothing.

    ``pool_sharded`` (default: environment KNNSVC_POOL_SHARD=1; needs a process group, one process per GPU; BASELINE
    cfg 4): EVERY rank must make this call with the same arguments.  The target pool's files are encoded in contiguous
    shares over the ranks, every rank searches the (replicated) query frames in its own shard and the pool's features /
    f0 / harmonics are all-gathered once (rank order = file order, so rows mean what they mean on one GPU).
      * ``share_items=False`` (single file): the per-shard top-32 lists are all-gathered and merged on every rank; every
        rank then holds the same neighbours, runs the same later stages and returns the same dicts.
      * ``share_items=True`` (dataset mode, ``bulk_match``): the source speaker's files are encoded in contiguous shares
        too (features all-gathered), the query items are dealt round-robin over the ranks, ONE all-to-all hands each
        rank the per-shard lists of its own items only, and each rank runs the match bodies (and ``vocode_fn``) of its
        own items: the returned dicts hold this rank's items."""
    import torch.distributed as tdist
    if ext is None:                  # refused before any file is read
        ext = Extensions.from_reference(topk=topk, use_topk=use_topk, use_vad=use_vad, vad_trigger_level=vad_trigger_level,
                                        f0_shift=f0_shift, transpose=transpose)
    target_duration = resolve_target_duration(target_duration)
    tune = resolve_tune(tune)
    if target_duration is not None and src_dataset_path is not None:
        raise ValueError("target_duration applies to a single source file: one duration for a dataset of utterances means nothing")
    refuse_duration_with_envelope([target_duration], ext)
    if pool_sharded is None:         # by environment: only when there is more than one rank to shard over
        pool_sharded = os.environ.get("KNNSVC_POOL_SHARD") == "1" and kdist.world()[1] > 1
    pool_sharded = bool(pool_sharded) and tdist.is_available() and tdist.is_initialized()   # explicit True: any group, even 1 rank
    share_items = bool(share_items) and pool_sharded
    assert prioritize_f0, "prioritize_f0=False is unsupported by the reference (ddsp_prematch_dataset.py:1375)"
    if "wavlm_only" not in ckpt_type and "no_harm_no_amp" not in ckpt_type and "mix" not in ckpt_type:
        raise NotImplementedError(ckpt_type)
    # the layer weighting (ddsp_prematch_dataset.py:349-350).  matching == synth features on the live path (ddsp_matcher.py:88-89,
    # 319: both the one-hot on layer 6).  Two DIFFERENT weightings mean two feature sets per target file: the pool is then encoded
    # once per weighting (the reference mixes both from one forward; this case is never taken live — correctness, not speed)
    mix_m, mix_s = _mix_of(match_weights, wavlm), _mix_of(synth_weights, wavlm)
    wavlm.set_layer_mix(mix_m)
    if src_dataset_path is None:
        assert os.path.isfile(src_wav_file)
    if target_duration is not None:  # the ratio is refused before anything is encoded
        duration_plan(frames_of(len(load_utterance(src_wav_file)[0]), wavlm), target_duration, item=str(src_wav_file))
    query_pool, _, _, _, query_f0_pool, _ = get_complete_spk_pool(src_wav_file, wavlm, device=device,
                                                                  shard_files=share_items, gather=share_items)
    if target_duration is not None:
        (key,) = list(query_pool)
        ft, f0 = stretch_queries([query_pool[key]], [query_f0_pool[key]], [target_duration])
        query_pool, query_f0_pool = {key: ft[0]}, {key: f0[0]}      # (new dicts: the pool store's entries stay as they are)
    if tgt_dataset_path is None:
        assert os.path.isfile(ref_wav_file)
    matching_pool, _synth, _audio, _spec, f0_pool, harm_pool = get_complete_spk_pool(
        ref_wav_file, wavlm, device=device, duration_limit=duration_limit, shard_files=pool_sharded, vad_trigger_level=ext.vad_level)
    keys = list(matching_pool)
    E = wavlm.E
    cat = lambda pool, shape: (torch.cat([pool[k] for k in keys], 0).contiguous() if keys
                               else torch.empty(shape, device=wavlm.device, dtype=torch.float32))
    matching_list, matching_f0, harmonics_list = cat(matching_pool, (0, E)), cat(f0_pool, (0,)), cat(harm_pool, (0, C.N_HARM))
    synth_list = None
    if mix_m != mix_s:
        wavlm.set_layer_mix(mix_s)
        try:
            # (a sharded pool: this rank's share again, under the synthesis weighting; all-gathered below like the matching features —
            #  the search only ever sees the matching features, the gathers and the smoothness weights read the synthesis ones)
            _m, synth_pool, _a2, _s2, _f2, _h2 = get_complete_spk_pool(ref_wav_file, wavlm, device=device, duration_limit=duration_limit,
                                                                       shard_files=pool_sharded, vad_trigger_level=ext.vad_level)
        finally:
            wavlm.set_layer_mix(mix_m)
        assert list(synth_pool) == keys
        synth_list = cat(synth_pool, (0, E))
        assert synth_list.shape == matching_list.shape
    shard = None
    if pool_sharded:
        shard = matching_list                                      # this rank's rows, searched locally
        counts = kdist.shard_rows(shard.shape[0], shard.device)
        if min(counts) < C.KNN_K:
            raise ops.KnnSvcError(f"pool shards {counts}: every rank needs at least {C.KNN_K} pool frames")
        matching_list = kdist.all_gather_rows_var(shard, counts)
        matching_f0 = kdist.all_gather_rows_var(matching_f0, counts)
        harmonics_list = kdist.all_gather_rows_var(harmonics_list, counts)
        if synth_list is not None:
            synth_list = kdist.all_gather_rows_var(synth_list, counts)

    out_c, harm_c, audio_c, f0_c = {}, {}, {}, {}
    items = [item for item in query_pool
             if required_subset is None or
             os.path.basename(item).split(".")[0] + "/" + os.path.basename(ref_wav_file) in required_subset]
    all_items = items

    def run():
        items = all_items
        nn = {}
        nn_ready = {}                 # item -> event of the kNN-stream search that produced nn[item]
        if shard is not None and share_items:
            # one search of ALL items' frames in every shard, one all-to-all: each rank gets the lists of its own items
            rank, ws = kdist.world()
            owned = [[it for j, it in enumerate(items) if j % ws == r] for r in range(ws)]      # == dist.my_share, per rank
            order = [it for part in owned for it in part]
            if order:
                q_all = torch.cat([query_pool[it] for it in order], 0).contiguous()
                rows = [sum(query_pool[it].shape[0] for it in part) for part in owned]
                mine_idx = kdist.sharded_knn_owned(q_all, rows, shard, C.KNN_K, counts=counts)[0]
                r0 = 0
                for it in owned[rank]:
                    n = query_pool[it].shape[0]
                    nn[it] = mine_idx[r0:r0 + n].contiguous()
                    r0 += n
            kdist.raise_if_any_nan()
            items = owned[rank]
            if matching_list.is_cuda:
                tok = ordering_token(matching_list.device)
                nn_ready.update({it: tok for it in nn})
        elif shard is not None:          # collectives first, in item order on every rank; the match bodies then need none
            for item in items:
                nn[item] = kdist.sharded_knn(query_pool[item].contiguous(), shard, C.KNN_K, replicated=True, counts=counts)[0]
            kdist.raise_if_any_nan()
            if matching_list.is_cuda:
                tok = ordering_token(matching_list.device)
                nn_ready.update({it: tok for it in nn})
        # the per-item bodies are independent chains of mostly single-workgroup kernels: three at a time, each on
        # its own pair of streams (pipeline.LanePipeline); the NaN flags of their kNN searches are read once at the end
        flags = []
        prep = prepare_pool(matching_list, split=shard is None) if len(items) > 1 else None
        if shard is None and len(items) > 1:
            # searches over the frames of SEVERAL items at a time (the reference searches 20 rows at a time,
            # ddsp_prematch_dataset.py:1195-1206; rows are independent): a [~3000, 1024] x [Np, 1024] product runs the matrix cores
            # 3-4 x as efficiently as one ~300-row search per utterance
            g_nn, g_ready = grouped_knn(items, query_pool, matching_list, prep, flags)
            nn.update(g_nn); nn_ready.update(g_ready)
        voice = types.SimpleNamespace(feats=matching_list, f0=matching_f0, harm=harmonics_list, prep=prep, synth=synth_list)
        own = SourceKnobs(f0_shift=ext.f0_shift, transpose=ext.transpose, tune=tune)          # (checked with the record)
        body, body_many = match_bodies(lambda it: (query_pool[it], query_f0_pool[it]), [voice], ckpt_type, post_opt, [(nn, nn_ready)],
                                       flags, lambda it: own, topk=ext.topk)
        # match bodies in flight at once (each is a chain of single-workgroup recurrences: more lanes = more of them side by side);
        # KNNSVC_MATCH=segmented (unsharded pool, several items): batches of KNNSVC_MATCH_BATCH items, each one body_many on a lane
        lanes = min(int(os.environ.get("KNNSVC_MATCH_LANES", "3")), len(items))
        tail = None
        if vocode_fn is not None and len(items) > 0:
            assert waves_out is not None
            # (load_utterance: mono, 16 kHz — the waveform the encoder received)
            wave = vocoding_tail(vocode_fn, items, lambda it: torch.from_numpy(load_utterance(it)[0]).to(matching_list.device))
            tail = lambda item, r: r + (wave(item, r),)
        results = run_match_bodies(items, body, body_many, tail, device=matching_list.device, lanes=lanes,
                                   match=match_mode() if shard is None else "lanes")
        if tail is not None:
            for item, r in zip(items, results):
                waves_out[item] = r[3]
            results = [r[:3] for r in results]
        for f in flags:
            ops.raise_if_nan(f)
        return items, results

    # a candidate-buffer overflow of the fused kNN route (reported by the deferred flags) repeats the searches and the bodies on
    # the dot-matrix route; under a process group every rank sees it together (dist.raise_if_any_nan)
    items, results = ops.retry_on_overflow(run)
    for item, (of, hw, sf0) in zip(items, results):
        out_c[item] = of; audio_c[item] = None; f0_c[item] = sf0
        if hw is not None:
            harm_c[item] = hw
    if "wavlm_only" in ckpt_type or "no_harm_no_amp" in ckpt_type:
        return out_c, audio_c, f0_c
    return out_c, harm_c, audio_c, f0_c
