"""Many-to-one batched conversion and a request queue (BASELINE cfg 5: many concurrent source clips against one
resident target pool).  The reference has no equivalent: its loops convert one utterance at a time and rebuild the target pool on
every call (ddsp_matcher.py:1073-1150, ddsp_prematch_dataset.py:1086-1134).  Everything here is host-side orchestration of the same
kernels, in the same order per utterance, as ``special_match`` / ``bulk_match`` — an utterance converted in a batch equals the same
utterance converted alone up to the rounding of the batch-wide power-of-two operand scales of the f16x2 GEMMs (range slots): bit
for bit with the small test models and on most full-size sources, <= 1e-6 otherwise (``tests/test_gpu_product.py``).

  TargetVoice      the pool of one target speaker, resident in HBM: features / f0 / harmonics, row norms, the f16x2 image the
                   kNN reads — built once (get_complete_spk_pool), reused by every request.
  BatchConverter   one batch of sources through the pipeline: batched encoder chunks (hipGraph buckets), batched f0 / side
                   features, kNN searches over the frames of several sources at a time on a stream of their own
                   (matching.grouped_knn), match bodies on lane streams, the generator as the tail stage (pipeline.LanePipeline).
                   No host synchronisation between the first launch and the last; the deferred kNN flags are read once.
                   Given 2 to 4 TargetVoice it converts towards a weighted mix of them (matching.match_features_blend), with
                   weights per converter, per source or per request.
  RequestQueue     dynamic batching for a serving process: ``submit`` returns a Future; one worker thread drains the queue into
                   batches (up to ``max_batch`` requests, waiting at most ``max_wait_ms`` for the batch to fill) and runs them
                   through a BatchConverter.  One worker per GPU: a hipGraph owns its buffers, so the same encoder / generator
                   graph must not be replayed from two host threads.

Several GPUs (one process per GPU): sources are independent — deal them over the ranks (``dist.my_share``) and give every rank
the same TargetVoice; when the pool itself is too large or too slow to encode on one GPU, use
``match_at_inference_time(pool_sharded=True, share_items=True)`` (``bulk_match`` with KNNSVC_POOL_SHARD=1), which shards the pool
rows and merges the per-shard lists over RCCL.
"""
from __future__ import annotations

import os
import queue
import threading
from concurrent.futures import Future
from pathlib import Path

import numpy as np
import torch

from . import audio_io, config as C, ops
from . import matching as M
from .matcher import Tail, VoiceTail
from .options import Extensions, SourceKnobs, per_item


class TargetVoice:
    """The resident pool of one target speaker (a file, or a folder of files; ``duration_limit`` in seconds as --dur_limit).
    ``vad_trigger_level``: the files are trimmed of the silence at both ends with that trigger level before they are encoded
    (matching.get_complete_spk_pool; None: left whole).  Every BatchConverter on this voice then matches against the trimmed pool."""

    def __init__(self, vc, ref_path, duration_limit=None, vad_trigger_level=None):
        self.ref_path = str(ref_path)
        self.ref_id = os.path.basename(self.ref_path).split(".")[0]
        with torch.inference_mode():
            vc.wavlm.set_layer_mix(M._mix_of(vc.weighting, vc.wavlm))
            mp, _s, _a, _spec, f0p, hp = M.get_complete_spk_pool(Path(ref_path), vc.wavlm, device=vc.device,
                                                                 duration_limit=duration_limit,
                                                                 vad_trigger_level=0 if vad_trigger_level is None else vad_trigger_level)
            keys = list(mp)
            self.files = keys
            self.feats = torch.cat([mp[k] for k in keys], 0).contiguous()
            self.f0 = torch.cat([f0p[k] for k in keys], 0).contiguous()
            self.harm = torch.cat([hp[k] for k in keys], 0).contiguous()
            if self.feats.shape[0] < C.KNN_K:
                raise ops.KnnSvcError(f"target pool has {self.feats.shape[0]} frames; the search needs at least {C.KNN_K}")
            self.prep = M.prepare_pool(self.feats)           # row norms + the split image of the kNN GEMM: once per voice

    @classmethod
    def from_clips(cls, vc, clips, name: str = "target"):
        """The same pool from audio already in memory: clips = [(wav [L] float32 16 kHz mono, f0 [L // 320 + 1]), ...]."""
        self = cls.__new__(cls)
        self.ref_path, self.ref_id, self.files = name, name, [f"{name}#{i}" for i in range(len(clips))]
        dev = vc.device
        with torch.inference_mode():
            vc.wavlm.set_layer_mix(M._mix_of(vc.weighting, vc.wavlm))
            g = lambda a: (a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))).to(dev)
            feats, f0s, harms = [], [], []
            for b in range(0, len(clips), 32):
                ws = [g(w).reshape(-1) for w, _ in clips[b:b + 32]]
                fs = vc.wavlm.encode_many(ws, max_batch=32, pow2_batches=True)
                sides = M.side_features_many(ws, [f for _, f in clips[b:b + 32]], [ft.shape[0] for ft in fs])
                feats += fs; f0s += [t[0] for t in sides]; harms += [t[1] for t in sides]
            from .wavlm import cat_rows
            self.feats = cat_rows(feats).contiguous()
            self.f0, self.harm = (torch.cat(x, 0).contiguous() for x in (f0s, harms))
            if self.feats.shape[0] < C.KNN_K:
                raise ops.KnnSvcError(f"target pool has {self.feats.shape[0]} frames; the search needs at least {C.KNN_K}")
            self.prep = M.prepare_pool(self.feats)
        return self

    @property
    def frames(self) -> int:
        return int(self.feats.shape[0])


class BatchConverter:
    def __init__(self, vc, target: TargetVoice, ckpt_type: str = "mix", post_opt: str = "post_opt_0.2", lanes: int | None = None,
                 max_encode_batch: int = 32, match: str | None = None, match_batch: int | None = None,
                 loudness_db: float | None = None, topk: int | None = None, f0_shift: str | None = None,
                 transpose: float | None = None, envelope_mix: float | None = None, peak_db: float | None = None,
                 ext: Extensions | None = None, blend=None, tune=None, harmony=None):
        # ``target``: one TargetVoice, or a sequence of 2 to 4 of them: the sources are then converted towards a weighted mix of
        # those voices (matching.match_features_blend; include/knnsvc_hip.h "Voice blend"), ``blend`` being the weights a source
        # gets unless a request says otherwise (blend_of; None: equal weights).  Refused before anything else: a sequence of
        # another length, ``blend`` with a single voice, a blend under KNNSVC_POOL_SHARD=1.
        self.voices = list(target) if isinstance(target, (list, tuple)) else None
        if self.voices is None:
            if blend is not None:
                raise ValueError("blend needs several target voices: pass a sequence of 2 to 4 TargetVoice as the target")
            self.blend = None
        else:
            self.blend = M.resolve_blend(blend, len(self.voices))
            M.refuse_blend_when_sharded()
        # ``tune``: the pitch correction a source gets unless a request says otherwise (tune_of; an options.Tuning, a scale such as
        # "A:minor", or None / "off": none; include/knnsvc_hip.h "Pitch correction")
        self.tune = M.resolve_tune(tune)
        # ``harmony``: the harmony parts a source gets unless a request says otherwise (harmony_of; an options.Harmony, or None /
        # "off": none; include/knnsvc_hip.h "Harmony voice").  Whether it names a scale, or the source's ``tune`` does, is checked
        # per source at the door of ``convert``.
        self.harmony = M.resolve_harmony(harmony)
        # the extension knobs, checked before anything else (options.py; None: off): ``loudness_db``, ``envelope_mix`` and
        # ``peak_db`` are part of the tail, on the tail's stream, enqueue-only, and apply to every request of a RequestQueue in
        # front of this converter; ``f0_shift`` / ``transpose`` are what a source gets unless a request says otherwise (pitch_of).
        # ``ext``: the record already built by the caller (many_to_one); the six arguments are then not read.
        self.ext = ext if ext is not None else Extensions.from_serving(loudness_db=loudness_db, topk=topk, f0_shift=f0_shift,
                                                                       transpose=transpose, envelope_mix=envelope_mix, peak_db=peak_db)
        if "wavlm_only_original" in ckpt_type:
            raise NotImplementedError("wavlm_only_original needs hifigan/models.py, absent upstream")
        self.vc, self.target, self.ckpt_type, self.post_opt = vc, target, ckpt_type, post_opt
        self.f0only = "wavlm_only" in ckpt_type or "no_harm_no_amp" in ckpt_type
        self.lanes = lanes if lanes is not None else int(os.environ.get("KNNSVC_MATCH_LANES", "3"))
        self.max_encode_batch = max_encode_batch
        # the match stage of a batch: "lanes" (default; one match body per source on the lane streams) or "segmented" (the sources
        # in order, in batches of match_batch, each batch ONE stacked match body: matching.match_features_many).  Defaults from
        # KNNSVC_MATCH / KNNSVC_MATCH_BATCH.
        self.match = M.match_mode(match)
        self.match_batch = M.match_batch_size(match_batch)

    def _load(self, src, check=False):
        """A request is a path, or (wav [L] float32 16 kHz mono as array / tensor, f0 [L // 320 + 1] or None).
        -> (wav on the device, f0 host array or device tensor)."""
        dev = self.vc.device
        if isinstance(src, (str, os.PathLike)):
            w, f0 = M.load_utterance(src)                    # resamples, reads or computes + caches <stem>_f0.npy
            return torch.from_numpy(w).to(dev), f0
        w, f0 = src
        w = w if isinstance(w, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(w, dtype=np.float32))
        # checked on the RAW input, before anything flattens it or runs on it: a [2, L] stereo array would otherwise be converted
        # as one 2L-sample mono clip, and Harvest would run on NaN samples before the finiteness check
        if w.dim() == 2 and 1 in w.shape:
            w = w.reshape(-1)                                # [1, L] / [L, 1]: mono with a channel axis (torchaudio.load's shape)
        if w.dim() != 1:
            raise ValueError(f"request: expected a mono waveform [L], got shape {tuple(w.shape)}")
        w = w.to(dev).float()
        if check and not bool(torch.isfinite(w).all()):      # (one small host read per request: a server checks its inputs at the door)
            raise ValueError("request: the waveform contains NaN or infinite samples")
        if f0 is None:
            f0 = ops.f0_harvest(w)                           # Harvest on the GPU (csrc/harvest.hip), as load_utterance does
        elif not isinstance(f0, torch.Tensor):
            f0 = np.ascontiguousarray(f0, dtype=np.float32)
        return w, f0

    def load_checked(self, src):
        """_load + the checks that do not need the encoder: a request that fails them fails alone (RequestQueue), before it can
        take a batch down with it.  -> (wav, f0)."""
        w, f0 = self._load(src, check=True)          # shape and finiteness are checked on the raw input, before Harvest runs on it
        if isinstance(src, (str, os.PathLike)) and not bool(torch.isfinite(w).all()):
            raise ValueError("request: the waveform contains NaN or infinite samples")
        T = M.frames_of(int(w.shape[0]), self.vc.wavlm)
        if T < 1:
            raise ValueError(f"request: expected a mono waveform of at least one frame, got shape {tuple(w.shape)}")
        if not (len(f0) >= T and len(f0) - T <= 1):
            raise ValueError(f"request: f0 has {len(f0)} frames for a waveform of {T} frames (expected {T} or {T + 1})")
        return w, f0

    def pitch_of(self, f0_shift=None, transpose=None, n=None):
        """Per-source ``f0_shift`` / ``transpose`` (a value for all, or one per source; None entries: this converter's defaults)
        as checked lists of ``n`` values each; ``n`` None: one checked pair."""
        if n is None:
            per = (self.ext.f0_shift if f0_shift is None else f0_shift, self.ext.transpose if transpose is None else transpose)
        else:
            per = [per_item(f0_shift, n, "f0_shift", default=self.ext.f0_shift),
                   per_item(transpose, n, "transpose", default=self.ext.transpose)]
        M.resolve_f0_shift(*per, n)
        return per

    def duration_of(self, target_duration=None, n=None):
        """``target_duration`` (seconds; a value for all sources, or one per source; None: off) checked
        (matching.resolve_target_duration) and held against this converter's envelope mix, which excludes it -> a list of
        ``n`` entries; ``n`` None: one checked value."""
        d = M.resolve_target_duration(target_duration, n)
        M.refuse_duration_with_envelope([d] if n is None else d, self.ext)
        return d

    def blend_of(self, blend=None, n=None):
        """Per-source blend weights (a vector for all sources, or one entry per source; None entries: this converter's default)
        checked and normalised (matching.resolve_blend) -> a list of ``n`` tuples; ``n`` None: one tuple.  With a single target
        voice there is nothing to blend: None (or ``n`` Nones) when no weights are given, ValueError when some are."""
        if self.voices is None:
            if blend is not None and not (isinstance(blend, (list, tuple)) and all(b is None for b in blend)):
                raise ValueError("blend needs several target voices: this converter has a single TargetVoice")
            return None
        one = lambda b: M.resolve_blend(b, len(self.voices))
        if n is None:
            return self.blend if blend is None else one(blend)
        return per_item(blend, n, "blend", one, default=self.blend, is_list=M.blend_per_item, unit="weight vectors")

    def tune_of(self, tune=None, n=None):
        """Per-source pitch correction (a value for all sources, or one per source; None entries: this converter's default,
        "off": none for that source) checked (matching.resolve_tune) -> a list of ``n`` entries (options.Tuning or None);
        ``n`` None: one checked value."""
        if n is None:
            return self.tune if tune is None else M.resolve_tune(tune)
        return [self.tune if t is None else t for t in M.resolve_tune(tune, n)]

    def harmony_of(self, harmony=None, tunes=None, n=None):
        """Per-source harmony (a value for all sources, or one per source; None entries: this converter's default, "off": none
        for that source) checked (matching.resolve_harmony) against the source's resolved ``tunes`` entry, which names the scale
        and tuning frequency where the harmony leaves them open -> a list of ``n`` entries, each None or (the options.Harmony,
        its options.HarmonyShift per part); ``n`` None: one entry for the single ``tunes`` value."""
        if n is None:
            return M.harmony_of(self.harmony if harmony is None else M.resolve_harmony(harmony), tunes)
        own = [self.harmony if h is None else h for h in M.resolve_harmony(harmony, n)]
        return [M.harmony_of(h, t) for h, t in zip(own, tunes)]

    def plan_duration(self, w, target_duration, item=None):
        """matching.duration_plan of a loaded source waveform (its frame count follows from its length: nothing is encoded)."""
        return M.duration_plan(M.frames_of(int(w.shape[0]), self.vc.wavlm), target_duration, item=item)

    @torch.inference_mode()
    def convert(self, sources, loaded=None, f0_shift=None, transpose=None, target_duration=None, blend=None, tune=None,
                harmony=None, stems=False) -> list:
        """-> one waveform tensor [T_i * 320] per source, in order.  ``loaded``: the sources already through load_checked.
        ``f0_shift`` / ``transpose``: for all sources or one per source (None: the converter's defaults); one batch may mix
        them on both match routes, each source's interval is chosen on the device.  ``target_duration`` (seconds): for all
        sources or one per source (None: off): that source's features and f0 are re-timed behind the encoder
        (matching.stretch_queries, one launch for the batch) and its waveform has matching.duration_plan's T_out * 320
        samples; sources with and without one share a batch.  ``blend`` (a converter with several target voices): the
        weights of the voices, for all sources or one vector per source (None: the converter's default); one batch may mix
        weight vectors on both match routes ("lanes": one blend per source, "segmented": one blend launch per batch).
        ``tune``: the pitch correction, for all sources or one entry per source (an options.Tuning or a scale; None: the
        converter's default, "off": none): that source's shifted f0 is snapped towards the key inside its match, on both routes;
        one batch may mix keys, and sources with and without one share a batch.
        ``harmony``: harmony parts, for all sources or one entry per source (an options.Harmony; None: the converter's default,
        "off": none).  A source with P parts becomes 1 + P items of the match stage that share its encoder output, its re-timed
        query and, per target voice, its ONE neighbour search; every part runs its own match body with the source's knobs and
        its own options.HarmonyShift (on the segmented route the parts are further segments), then the per-voice half of the
        tail (generator, envelope mix).  The voices are mixed (ops.mix_waves, gains 10^(dB / 20), lead first) and the per-output
        half (loudness, ceiling) and the finiteness check run on the mix.  The lead is bit-identical to the source's conversion
        without a harmony.  ``stems``: -> per source the list [mix, lead, part_1, ...] of waveforms instead of the mix alone
        (the stems are the outputs of the per-voice half; a source without a harmony: [output, lead])."""
        modes, semis = self.pitch_of(f0_shift, transpose, len(sources))        # refused before a file is read
        durs = self.duration_of(target_duration, len(sources))
        mixes = self.blend_of(blend, len(sources))
        tunes = self.tune_of(tune, len(sources))
        knobs = [SourceKnobs(*k) for k in zip(modes, semis, durs, mixes or [None] * len(sources), tunes)]
        harms = self.harmony_of(harmony, tunes, len(sources))
        if len(sources) == 0:
            return []
        vc, voices = self.vc, self.voices or [self.target]
        dev = vc.device
        vc.wavlm.set_layer_mix(M._mix_of(vc.weighting, vc.wavlm))      # the shared encoder may have been left in another mix
        loaded = loaded if loaded is not None else [self._load(s) for s in sources]
        wavs = [w for w, _ in loaded]
        for i, d in enumerate(durs):                                   # a ratio out of bounds is refused before anything is encoded
            if d is not None:
                self.plan_duration(wavs[i], d, item=f"source {i}")
        feats = vc.wavlm.encode_many(wavs, max_batch=self.max_encode_batch, pow2_batches=True)
        f0s = []
        for (w, f0), ft in zip(loaded, feats):
            T = ft.shape[0]
            if not (abs(len(f0) - T) <= 1 and len(f0) >= T):
                raise ValueError(f"f0 has {len(f0)} frames for {T} feature frames")
            f0s.append(f0[:T].contiguous().to(dev) if isinstance(f0, torch.Tensor)
                       else torch.from_numpy(np.ascontiguousarray(f0[:T])).to(dev, non_blocking=True))
        feats, f0s = M.stretch_queries(feats, f0s, durs)               # in front of everything of the match stage
        # items of the match stage: source i is item i (its lead); the parts of the harmonised sources follow behind the leads
        n_src = len(sources)
        src_of, part_of, members = list(range(n_src)), [None] * n_src, [[i] for i in range(n_src)]
        for i, h in enumerate(harms):
            for shift in (h[1] if h is not None else ()):
                members[i].append(len(src_of)); src_of.append(i); part_of.append(shift)
        items = list(range(len(src_of)))
        leads = items[:n_src]
        qpool = {it: feats[src_of[it]] for it in items}
        # the reference does not forward post_opt to the f0-only generators (ddsp_matcher.py:970, 1102-1110)
        post_opt = "no_post_opt" if self.f0only else self.post_opt
        whole = Tail(vc, self.f0only, self.ext)
        source_of = lambda it: wavs[src_of[it]]
        tail = M.vocoding_tail(whole, items, source_of)
        # the items whose output is mixed (or handed out as a stem) stop behind the per-voice half of the tail
        halved = {it for it in items if stems or len(members[src_of[it]]) > 1}
        if halved:
            tail_whole, tail_voice = tail, M.vocoding_tail(VoiceTail(whole), items, source_of)
            tail = lambda item, r: (tail_voice if item in halved else tail_whole)(item, r)

        def run():
            # every voice that some source of the batch gives weight to (a single target: that one) is searched over the frames
            # of several sources at a time (grouped_knn) and matched on its own; a blend sits between the match bodies and the tail
            flags = []
            used = [len(items) > 1 and (mixes is None or any(m[v] != 0.0 for m in mixes)) for v in range(len(voices))]
            found = [M.grouped_knn(leads, qpool, vo.feats, vo.prep, flags) if u else ({}, {}) for vo, u in zip(voices, used)]
            for nn, ready in found:                          # a part reuses its lead's list: it is not searched again
                for it in items[n_src:]:
                    if src_of[it] in nn:
                        nn[it] = nn[src_of[it]]
                        if src_of[it] in ready:
                            ready[it] = ready[src_of[it]]
            body, body_many = M.match_bodies(lambda i: (qpool[i], f0s[src_of[i]]), voices, self.ckpt_type, post_opt, found, flags,
                                             lambda i: knobs[src_of[i]], topk=self.ext.topk,
                                             **(dict(parts=part_of.__getitem__) if len(items) > n_src else {}))
            ys = M.run_match_bodies(items, body, body_many, tail, device=dev, lanes=max(1, min(self.lanes, len(items))),
                                    match=self.match, match_batch=self.match_batch)
            outs = ys[:n_src]
            for i in range(n_src if halved else 0):
                if len(members[i]) > 1:
                    mix = ops.mix_waves([ys[it] for it in members[i]], harms[i][0].gains)
                    outs[i] = whole.per_output(mix)
                elif i in halved:                            # (stems of a source without parts: the lead stays as it is)
                    outs[i] = whole.per_output(ys[i].clone())
            peak = torch.stack([y.abs().max() for y in outs])
            for f in flags:
                ops.raise_if_nan(f)                          # one host read per search, after everything is enqueued
            vc._check_finite(peak)
            return [[outs[i]] + [ys[it] for it in members[i]] for i in range(n_src)] if stems else outs
        return ops.retry_on_overflow(run)

    def convert_files(self, src_files, converted_audio_dir=None, target_duration=None, blend=None, tune=None, harmony=None) -> list:
        """Paths in, files out: ``<dir or the source's folder>/<src>_to_<ref>_knn_<ckpt_type>_<post_opt>.wav`` (the single-file
        naming, ddsp_matcher.py:1015), PCM_32 16 kHz mono.  -> the written paths.  ``target_duration`` / ``blend`` / ``tune`` / ``harmony``: as ``convert``
        (the mix is written; the file name does not change).
        With several target voices ``<ref>`` is their ids joined by ``+`` (``<idA>+<idB>[+...]``); the weights are not in the name."""
        ys = self.convert([str(p) for p in src_files], target_duration=target_duration, **({} if blend is None else dict(blend=blend)),
                          **({} if tune is None else dict(tune=tune)), **({} if harmony is None else dict(harmony=harmony)))
        out = []
        for p, y in zip(src_files, ys):
            path = self.output_path(p, converted_audio_dir)
            Path(path).parent.mkdir(parents=True, exist_ok=True)
            out.append(audio_io.save_audio(path, y.detach().cpu().numpy(), sample_rate=16000))
        return out

    def output_path(self, src_file, converted_audio_dir=None) -> str:
        """Where ``convert_files`` writes the conversion of ``src_file``."""
        d = converted_audio_dir if converted_audio_dir is not None else str(Path(src_file).parent)
        ref_id = self.target.ref_id if self.voices is None else "+".join(v.ref_id for v in self.voices)
        return os.path.join(d, os.path.basename(str(src_file)).split(".")[0] + "_to_" + ref_id + f"_knn_{self.ckpt_type}_{self.post_opt}.wav")


class RequestQueue:
    """Dynamic batching in front of a BatchConverter.  ``submit(src)`` -> Future of the waveform (a CPU tensor).
    ``submit(src, transpose=, f0_shift=)``: the request's own transpose (semitones) / f0 shift mode instead of the converter's;
    ``submit(src, target_duration=)``: the length in seconds the request's conversion is re-timed to (BatchConverter.convert);
    ``submit(src, blend=)`` (a converter with several target voices): the request's own blend weights; a bad vector is refused
    at the door and fails alone; ``submit(src, tune=)``: the request's own pitch correction (an options.Tuning, a scale, or "off"
    under a converter whose default is on), refused at the door likewise; ``submit(src, harmony=)``: the request's own harmony
    parts (an options.Harmony, or "off"), refused at the door likewise.  Requests with different values share a batch.
    The converter's ``loudness_db``, ``envelope_mix`` and ``peak_db`` apply to every request (per-request values of those are
    not supported)."""

    def __init__(self, converter: BatchConverter, max_batch: int = 32, max_wait_ms: float = 5.0):
        self.conv, self.max_batch, self.max_wait = converter, int(max_batch), float(max_wait_ms) / 1e3
        self._q = queue.Queue()
        self._stop = False
        self.batches = []                                    # sizes of the batches run so far (observability / tests)
        self.isolated = 0                                    # batches that failed as a whole and were re-run request by request
        self._th = threading.Thread(target=self._loop, name="knnsvc-batcher", daemon=True)
        self._th.start()

    def submit(self, src, transpose=None, f0_shift=None, target_duration=None, blend=None, tune=None, harmony=None) -> Future:
        if self._stop:
            raise RuntimeError("RequestQueue is closed")
        fut = Future()
        own = {}                                             # a bad value is refused here, not in the worker
        if transpose is not None or f0_shift is not None:
            own["f0_shift"], own["transpose"] = self.conv.pitch_of(f0_shift, transpose)
        if target_duration is not None:
            own["target_duration"] = self.conv.duration_of(target_duration)
        if blend is not None:
            own["blend"] = self.conv.blend_of(blend)
        if tune is not None:
            own["tune"] = self.conv.tune_of(tune)
        if harmony is None:
            self._q.put((src, fut, SourceKnobs(**own)))
            return fut
        # a harmony travels beside the knobs, in an entry of its own; checked against the tune the request will be converted with
        harmony = M.resolve_harmony(harmony)
        self.conv.harmony_of(harmony, own.get("tune", self.conv.tune))
        self._q.put((src, fut, SourceKnobs(**own), harmony))
        return fut

    def _loop(self):
        dev = self.conv.vc.device
        if dev.type == "cuda" and dev.index is not None:     # a new host thread starts on device 0
            torch.cuda.set_device(dev)
        import time
        while True:
            first = self._q.get()
            if first is None:
                return
            batch = [first]
            deadline = time.monotonic() + self.max_wait       # ONE deadline per batch, set by its first request: a trickle of
            try:                                              # arrivals cannot hold it longer than max_wait_ms
                while len(batch) < self.max_batch:
                    nxt = self._q.get(timeout=max(0.0, deadline - time.monotonic()))
                    if nxt is None:
                        self._q.put(None)                    # finish this batch, then stop
                        break
                    batch.append(nxt)
            except queue.Empty:
                pass
            self.batches.append(len(batch))
            self._run(batch)

    def _run(self, batch):
        """One batch; a request that cannot be loaded, or whose data makes the conversion fail (a NaN source, an f0 track of the
        wrong length, a target duration out of proportion to its length), fails ALONE: the others of its batch are converted
        without it.  An entry is (source, Future, SourceKnobs: the request's own values, None where it has none[, the request's own
        harmony]); a knob is
        passed on to ``convert`` only when a request of the batch carries it (``f0_shift`` and ``transpose`` together), so a batch
        in which no request carries values of its own is converted as it always was."""
        good, loaded = [], []
        for s, fut, own, *harm in batch:
            try:
                ld = self.conv.load_checked(s)
                if own.target_duration is not None:          # needs the loaded source: refused here, before the batch is formed
                    self.conv.plan_duration(ld[0], own.target_duration, item="request")
                loaded.append(ld)
                good.append((s, fut, own, harm[0] if harm else None))
            except BaseException as e:
                fut.set_exception(e)
        if not good:
            return
        carried = [names for names in (("f0_shift", "transpose"), ("target_duration",), ("blend",), ("tune",))
                   if any(getattr(own, k) is not None for _s, _f, own, _h in good for k in names)]
        harmonised = any(h is not None for _s, _f, _own, h in good)
        kwargs = lambda gs: dict({k: [getattr(own, k) for _s, _f, own, _h in gs] for names in carried for k in names},
                                 **(dict(harmony=[h for _s, _f, _own, h in gs]) if harmonised else {}))
        try:
            ys = self.conv.convert([g[0] for g in good], loaded=loaded, **kwargs(good))
            for (_s, fut, _own, _h), y in zip(good, ys):
                fut.set_result(y.detach().cpu())
            return
        except BaseException as e:
            if len(good) == 1:
                good[0][1].set_exception(e)
                return
        self.isolated += 1
        for g, ld in zip(good, loaded):                       # the batch failed as a whole: find the offender(s) one by one
            try:
                g[1].set_result(self.conv.convert([g[0]], loaded=[ld], **kwargs([g]))[0].detach().cpu())
            except BaseException as e:
                g[1].set_exception(e)

    def close(self):
        self._stop = True
        self._q.put(None)
        self._th.join()
