"""``KNeighborsVC`` — the orchestrator object the reference's entry points hand out.

Mirror of ddsp_matcher.py:303-1155 restricted to its live methods: ``vocode``
(:375-406), ``special_match`` (:937-1023) and ``bulk_match`` (:1027-1155), with the
same argument names and output file naming.  The arguments upstream accepts and drops (``topk``, ``tgt_loudness_db``,
``vad_trigger_level``) and the ones it does not have (``f0_shift``, ``transpose``, ``envelope_mix``, ``peak_db``, ``tune``) are the
extension knobs: knn_svc_amd/options.py has the table of what each does and when it is ignored; every entry point below folds
them into one ``options.Extensions`` first.  ``audio_io.save_audio`` keeps the reference's peak rule — a waveform whose peak
exceeds 1 is divided by it — so a clip normalised past full scale is written lower than asked unless ``peak_db`` holds its
peaks under a ceiling first.  Other differences that are deliberate: ``special_match`` returns
the waveform instead of calling ``sys.exit()`` after saving (the CLI exits 0, the
observable behaviour), and ``bulk_match`` does not ``rm -rf`` a hard-coded cache
directory (ddsp_matcher.py:1066-1068).
"""
from __future__ import annotations

import csv
import os
from pathlib import Path

import torch

from . import audio_io, config as C, dist as kdist, ops
from .matching import (harmony_of, load_utterance, match_at_inference_time, refuse_duration_with_envelope, resolve_harmony,
                       resolve_target_duration, resolve_tune)
from .options import Extensions
from .vocoder import Vocoder
from .wavlm import WavLMEncoder

# one-hot on layer 6 of 25 (ddsp_matcher.py:88-89, knnvc_utils.py:3-6)
SPEAKER_INFORMATION_WEIGHTS = [1.0 if i == C.MATCH_LAYER else 0.0 for i in range(25)]


class Tail:
    """What follows the match stage for one utterance, enqueue only (no host sync), on the current stream: the ``vocode_fn`` of the
    stream pipeline and the body of ``vocode``.  Fixed order: generator (``f0only``: without the harmonics); envelope mix
    (``ext.envelope_mix`` > 0: the shape of ``src_wav``'s envelope, first because it changes the level); loudness
    (``ext.loudness_db``: measured and scaled to that level); peak ceiling (``ext.peak_db``: last, so that what is written respects
    it).  The first two in place (``Vocoder.forward`` hands out a copy).  ``needs_source``: whether a caller has to pass
    ``src_wav``, the utterance's source as the encoder received it (1-D fp32 on the device, 16 kHz mono)."""

    def __init__(self, vc, f0only: bool, ext: Extensions):
        self.vc, self.f0only, self.ext = vc, f0only, ext
        self.needs_source = ext.envelope_mix > 0

    def __call__(self, out_feats, shifted_f0, harm, src_wav=None):
        return self.per_output(self.per_voice(out_feats, shifted_f0, harm, src_wav))

    def per_voice(self, out_feats, shifted_f0, harm, src_wav=None):
        """The half that runs once per voice of an output (the lead, and every harmony part): generator, envelope mix."""
        vc, ext = self.vc, self.ext
        y = vc.hifigan.forward(out_feats.float(), shifted_f0.reshape(-1).float(), None if self.f0only or harm is None else harm.float())
        if self.needs_source:
            ops.envelope_mix(y, src_wav, ext.envelope_mix, hop=vc.hop_length, out=y)
        return y

    def per_output(self, y):
        """The half that runs once per output, on one voice or on the mix of several (ops.mix_waves): loudness, ceiling.  The
        loudness in place."""
        vc, ext = self.vc, self.ext
        if ext.loudness_db is not None:
            ops.normalize_loudness(y, ext.loudness_db, vc.sr, out=y)
        if ext.peak_db is not None:
            y = ops.limit_peak(y, ext.peak_db, vc.sr)          # out of place: the parallel launch
        return y


class VoiceTail:
    """The per-voice half of a ``Tail`` as a ``vocode_fn`` of its own: what a voice that is going to be mixed with others (a lead
    and its harmony parts) runs behind its match body."""

    def __init__(self, tail: Tail):
        self.tail, self.needs_source = tail, tail.needs_source

    def __call__(self, out_feats, shifted_f0, harm, src_wav=None):
        return self.tail.per_voice(out_feats, shifted_f0, harm, src_wav)


class KNeighborsVC:
    def __init__(self, wavlm: WavLMEncoder, hifigan: Vocoder, hifigan_cfg: dict, device="cuda") -> None:
        self.wavlm = wavlm
        self.hifigan = hifigan
        self.h = hifigan_cfg
        self.device = torch.device(device)
        self.weighting = torch.zeros(wavlm.cfg["encoder_layers"] + 1)
        self.weighting[wavlm.n_layers] = 1.0
        self.sr = hifigan_cfg["sampling_rate"]
        self.hop_length = 320

    @torch.inference_mode()
    def vocode(self, c, f0=None, harmonics_out_feats_weighted=None, loudness_db=None, src_wav=None, envelope_mix=0.0, peak_db=None):
        """c (bs, seq_len, c_dim), f0 (bs, seq_len, 1), harmonics (bs, seq_len, 49) -> (bs, seq_len*320).
        ``loudness_db`` / ``envelope_mix`` / ``peak_db``: the tail's extension knobs (options.py).  ``src_wav``: the bs source
        waveforms (a [bs, L] tensor or a list of [L_b] tensors, 16 kHz mono as the encoder received them); needed when
        ``envelope_mix`` > 0."""
        ext = Extensions.from_serving(loudness_db=loudness_db, envelope_mix=envelope_mix, peak_db=peak_db)
        return self._vocode(Tail(self, harmonics_out_feats_weighted is None, ext), c, f0, harmonics_out_feats_weighted, src_wav)

    def _vocode(self, tail, c, f0, harm=None, src_wav=None):
        """``tail`` on every utterance of the batch, then one finiteness check."""
        if tail.needs_source and src_wav is None:
            raise ValueError("vocode: envelope_mix > 0 needs src_wav, the source waveforms")
        if f0 is None:
            raise NotImplementedError("the f0-free 'wavlm_only_original' generator (hifigan/models.py) is missing "
                                      "from the reference snapshot and unsupported")
        dev = self.device
        wav = torch.stack([tail(c[b].to(dev), f0[b].to(dev), None if harm is None else harm[b].to(dev),
                                src_wav[b].reshape(-1).float().to(dev) if tail.needs_source else None) for b in range(c.shape[0])], 0)
        self._check_finite(wav)
        return wav

    @staticmethod
    def _check_finite(wav):
        # operand scales follow the data (range slots), so a non-finite sample means a non-finite input or weight
        if not bool(torch.isfinite(wav).all()):
            raise ops.KnnSvcError("vocode: non-finite waveform (non-finite features, f0, harmonics or weights)")

    @staticmethod
    def blend_voices(ref_wav_file, blend_with=None, blend=None):
        """The references of a voice blend, checked before a file is read: ``[ref_wav_file, *blend_with]`` (``blend_with``: one
        path or a sequence of one to three) with ``blend`` as their weights (matching.resolve_blend; None: equal), or None
        without ``blend_with`` — ``blend`` alone is refused, as are more than four voices, a wrong count of weights and a blend
        under KNNSVC_POOL_SHARD=1."""
        from .matching import refuse_blend_when_sharded, resolve_blend
        if blend_with is None:
            if blend is not None:
                raise ValueError("blend needs several target voices: give the further references as blend_with")
            return None
        more = [blend_with] if isinstance(blend_with, (str, os.PathLike)) else list(blend_with)
        if not 1 <= len(more) <= 3:
            raise ValueError(f"blend_with takes one to three further references (four voices in all), got {len(more)}")
        resolve_blend(blend, 1 + len(more))
        refuse_blend_when_sharded()
        return [ref_wav_file] + more

    @torch.inference_mode()
    def special_match(self, src_wav_file, ref_wav_file, topk: int = 4, device=None, prioritize_f0=True,
                      ckpt_type="wavlm_only", tgt_loudness_db=-16, post_opt="no_post_opt", save=True, normalize_loudness=False,
                      use_topk=False, use_vad=False, vad_trigger_level=7, f0_shift="median", transpose=0.0, envelope_mix=0.0,
                      peak_db=None, target_duration=None, blend_with=None, blend=None, tune=None, harmony=None):
        """``harmony`` (an options.Harmony, None: off): 1 to 3 harmony parts — the lead's contour moved by scale degrees, sung by
        the same target voice from the source's one encoder pass and neighbour search, and mixed under the lead on the GPU
        (options.py has the semantics; its scale, or else ``tune``'s, names the key); through serving.TargetVoice and
        serving.BatchConverter, as a blend; the mix is returned and written, the file name does not change.  ``bulk_match``,
        ``match_at_inference_time`` and ``vocode`` do not take it: they return one feature set per source.
        ``tune`` (an options.Tuning, a scale such as "A:minor" or "chromatic", None: off): pitch correction — the shifted f0
        is snapped towards the notes of that key, the OUTPUT's key, on the GPU inside the match stage (matching.resolve_tune;
        options.py has the semantics); the file name does not change.  ``vocode`` does not take it: it starts behind the match
        stage, where ops.tune_f0_seg serves such callers.
        ``target_duration`` (seconds, None: off): the conversion re-timed to that length — the waveform has
        matching.duration_plan's T_out * 320 samples, the file name does not change; not with ``envelope_mix`` > 0.
        ``blend_with`` (one to three further reference files or folders) / ``blend`` (weights for ``[ref_wav_file, *blend_with]``,
        None: equal): the conversion goes towards that weighted mix of voices (``blend_voices``), through serving.TargetVoice and
        serving.BatchConverter; ``use_vad`` trims every voice's pool; the file is named ``<src>_to_<idA>+<idB>[+...]_knn_...``."""
        ext = Extensions.from_reference(topk, use_topk, tgt_loudness_db, normalize_loudness, use_vad, vad_trigger_level, f0_shift,
                                        transpose, envelope_mix, peak_db)          # refused before a file is read
        refuse_duration_with_envelope([resolve_target_duration(target_duration)], ext)
        tune = resolve_tune(tune)
        harmony = resolve_harmony(harmony)
        parts = harmony_of(harmony, tune)          # a harmony without a scale, its own or the tune's, is refused here
        refs = self.blend_voices(ref_wav_file, blend_with, blend)
        if refs is None and parts is not None:
            refs = [ref_wav_file]
        f0only = "wavlm_only" in ckpt_type or "no_harm_no_amp" in ckpt_type
        if "wavlm_only_original" in ckpt_type:
            raise NotImplementedError("wavlm_only_original needs hifigan/models.py, absent upstream")
        if refs is not None:
            from . import serving
            voices = [serving.TargetVoice(self, r, vad_trigger_level=ext.vad_level) for r in refs]
            conv = serving.BatchConverter(self, voices if len(voices) > 1 else voices[0], ckpt_type, post_opt, ext=ext, blend=blend,
                                          tune=tune, harmony=harmony)
            pred = conv.convert([str(src_wav_file)], target_duration=target_duration)[0]
            if save:
                out_file = conv.output_path(src_wav_file)
                print("->", out_file)
                audio_io.save_audio(out_file, pred.detach().cpu().numpy(), sample_rate=16000)
            return pred
        key = str(src_wav_file)
        # the reference does not forward post_opt to the f0-only generators (ddsp_matcher.py:970)
        res = match_at_inference_time(Path(src_wav_file), Path(ref_wav_file), self.wavlm, self.weighting, self.weighting,
                                      device=self.device, prioritize_f0=prioritize_f0, ckpt_type=ckpt_type, ext=ext,
                                      target_duration=target_duration, tune=tune, **({} if f0only else dict(post_opt=post_opt)))
        tail = Tail(self, f0only, ext)
        src = [torch.from_numpy(load_utterance(src_wav_file)[0])] if tail.needs_source else None
        pred = self._vocode(tail, res[0][key][None], res[-1][key][None, :, None], None if f0only else res[1][key][None], src).squeeze()
        src_id = os.path.basename(src_wav_file).split(".")[0]
        ref_id = os.path.basename(ref_wav_file).split(".")[0]
        out_file = str(Path(src_wav_file).parent) + "/" + src_id + "_to_" + ref_id + f"_knn_{ckpt_type}_{post_opt}.wav"
        if save:
            print("->", out_file)
            audio_io.save_audio(out_file, pred.detach().cpu().numpy(), sample_rate=16000)
        return pred

    @torch.inference_mode()
    def many_to_one(self, src_files, ref_wav_file, converted_audio_dir=None, ckpt_type="mix", post_opt="post_opt_0.2",
                    duration_limit=None, target=None, match=None, loudness_db=None, topk=None, vad_trigger_level=None,
                    f0_shift=None, transpose=None, envelope_mix=None, peak_db=None, target_duration=None, blend_with=None,
                    blend=None, tune=None, harmony=None):
        """BASELINE cfg 5 (no counterpart upstream: the reference would call ``special_match`` once per source and rebuild the
        target pool each time, ddsp_matcher.py:937-1023): MANY sources against ONE target pool that is built once and stays
        resident, all sources through the stream pipeline as one batch (knn_svc_amd/serving.py).  Under a process group the
        sources are dealt over the ranks (no collective).  ``target``: a serving.TargetVoice to reuse.  -> written paths (all
        ranks' on every rank), named like ``special_match``'s outputs.  ``match``: "lanes" | "segmented" (serving.BatchConverter; default
        from KNNSVC_MATCH).  ``loudness_db`` ... ``peak_db``: the extension knobs, None = off (options.Extensions.from_serving;
        ``vad_trigger_level`` is ignored when ``target`` is given).  ``target_duration``: seconds, one value for all sources or
        a list with one entry per source (None entries: off; serving.BatchConverter.convert).  ``blend_with`` (one to three
        further reference files or folders) / ``blend`` (weights for ``[ref_wav_file, *blend_with]``, None: equal): every source is
        converted towards that weighted mix of voices (``blend_voices``; each voice's pool is trimmed when ``vad_trigger_level``
        is given); ``target`` is then a sequence of TargetVoice to reuse, and the outputs are named ``<src>_to_<idA>+<idB>[+...]``.
        ``tune``: the pitch correction, one value for all sources or a list with one entry per source (an options.Tuning, a
        scale, None / "off": none; serving.BatchConverter.convert).  ``harmony``: harmony parts, one value for all sources or a list
        with one entry per source (an options.Harmony, None / "off": none; serving.BatchConverter.convert): the mix is written."""
        from . import serving
        ext = Extensions.from_serving(loudness_db, topk, vad_trigger_level, f0_shift, transpose, envelope_mix, peak_db)   # before a file is read
        refuse_duration_with_envelope(resolve_target_duration(target_duration, len(src_files)), ext)
        tunes = resolve_tune(tune, len(src_files))
        for h, t in zip(resolve_harmony(harmony, len(src_files)), tunes):
            harmony_of(h, t)
        # (voices handed in as ``target``: the converter checks the weights against them)
        refs = None if isinstance(target, (list, tuple)) else self.blend_voices(ref_wav_file, blend_with, blend)
        if target is None:
            target = serving.TargetVoice(self, ref_wav_file, duration_limit, vad_trigger_level=ext.vad_level) if refs is None else \
                [serving.TargetVoice(self, r, duration_limit, vad_trigger_level=ext.vad_level) for r in refs]
        mine = kdist.my_share([str(p) for p in src_files])
        if isinstance(target_duration, (list, tuple)):        # this rank's sources' own entries
            target_duration = kdist.my_share(list(target_duration))
        if isinstance(tune, (list, tuple)):
            tune = kdist.my_share(list(tune))
        if isinstance(harmony, (list, tuple)):
            harmony = kdist.my_share(list(harmony))
        written = serving.BatchConverter(self, target, ckpt_type, post_opt, match=match, ext=ext, blend=blend).convert_files(
            mine, converted_audio_dir, target_duration=target_duration, tune=tune, harmony=harmony)
        return kdist.gather_paths(written)

    @torch.inference_mode()
    def bulk_match(self, src_dataset_path, tgt_dataset_path, converted_audio_dir, topk: int = 4, device=None,
                   prioritize_f0=True, ckpt_type="mix", tgt_loudness_db=-16, required_subset_file=None,
                   post_opt="no_post_opt", duration_limit=None, normalize_loudness=False, use_topk=False, use_vad=False,
                   vad_trigger_level=7, f0_shift="median", transpose=0.0, envelope_mix=0.0, peak_db=None, tune=None):
        """``tune`` (an options.Tuning, a scale, None: off): pitch correction of every utterance's shifted f0 towards that key
        (``special_match``)."""
        ext = Extensions.from_reference(topk, use_topk, tgt_loudness_db, normalize_loudness, use_vad, vad_trigger_level, f0_shift,
                                        transpose, envelope_mix, peak_db)          # refused before a file is read
        tune = resolve_tune(tune)
        assert os.path.isdir(src_dataset_path) and os.path.isdir(tgt_dataset_path)
        Path(converted_audio_dir).mkdir(parents=True, exist_ok=True)
        spk = lambda root: sorted([p for p in Path(root).iterdir() if p.is_dir() and "f0_cache" not in os.path.basename(p)])
        src_spk, tgt_spk = spk(src_dataset_path), spk(tgt_dataset_path)
        if src_dataset_path != tgt_dataset_path:
            assert len(set(src_spk).intersection(set(tgt_spk))) == 0
        assert len(src_spk) > 0, [f"Are you sure {src_dataset_path} is a FOLDER containing speaker folders, i.e. dataset root"]
        assert len(tgt_spk) > 0, [f"Are you sure {tgt_dataset_path} is a FOLDER containing speaker folders, i.e. dataset root"]
        required = None
        if required_subset_file:
            with open(required_subset_file, "r") as fp:
                rows = list(csv.reader(fp, delimiter=",", quotechar='"'))
            required = [r[2] for i, r in enumerate(rows) if i != 0 and r[-1] == "0"]
        f0only = "wavlm_only" in ckpt_type or "no_harm_no_amp" in ckpt_type
        # Files are encoded and written by a small thread pool while the next speaker pair is on the GPU (a pair's 80 files cost
        # the host ~20 ms during which the device idled: 7 % of a cfg-3 run, tools/timeline_cmd.sh); the paths are collected in
        # order at the end, where a failed write raises.
        from concurrent.futures import ThreadPoolExecutor
        writer = ThreadPoolExecutor(max_workers=2, thread_name_prefix="knnsvc-writer")
        pending = []
        pairs = [(s, t) for i, s in enumerate(src_spk) for j, t in enumerate(tgt_spk)
                 if not (src_dataset_path == tgt_dataset_path and i == j)]
        # One process per GPU, two ways to share a dataset run, never both at once:
        #   * default: speaker pairs are independent (clip-DP) and are dealt round-robin over the ranks, every rank
        #     handles ITS pairs alone (pool_sharded=False: no collective may run, the other ranks are on other pairs);
        #   * KNNSVC_POOL_SHARD=1 (BASELINE cfg 4, pools too large / too slow for one GPU): EVERY rank walks EVERY pair
        #     in the same order, each pair's target pool and source files are encoded in shares over the ranks, the kNN
        #     is searched per shard, and the utterances of the pair are dealt over the ranks for matching + vocoding.
        rank, ws = kdist.world()
        shard = os.environ.get("KNNSVC_POOL_SHARD") == "1" and ws > 1
        my_pairs = pairs if shard else kdist.my_share(pairs)
        try:
            for s, t in my_pairs:
                print(f"{s} -> {t}")
                # the generator of every utterance is the tail stage of the match pipeline (same kernels and inputs as
                # `vocode` after the fact, ddsp_matcher.py:1114-1128, but enqueued under the next utterances' matching);
                # one finiteness check per speaker pair instead of one host sync per utterance; with normalize_loudness,
                # envelope_mix or peak_db the tail is generator + those stages, still enqueue-only.  The reference does not
                # forward post_opt to the f0-only generators (:1102-1110)
                preds = {}
                match_at_inference_time(Path(s), Path(t), self.wavlm, self.weighting, self.weighting, device=self.device,
                                        prioritize_f0=prioritize_f0, ckpt_type=ckpt_type, src_dataset_path=src_dataset_path,
                                        tgt_dataset_path=tgt_dataset_path, required_subset=required, duration_limit=duration_limit,
                                        pool_sharded=shard, share_items=shard, ext=ext, vocode_fn=Tail(self, f0only, ext),
                                        waves_out=preds, tune=tune, **({} if f0only else dict(post_opt=post_opt)))
                if preds:      # max |x| of a waveform is NaN / inf iff the waveform holds one
                    self._check_finite(torch.stack([p.abs().max() for p in preds.values()]))
                for k, pred in preds.items():
                    out = os.path.join(converted_audio_dir, os.path.basename(s), os.path.basename(k).split(".")[0],
                                       os.path.basename(t) + "." + os.path.basename(k).split(".")[-1])
                    Path(out).parent.mkdir(parents=True, exist_ok=True)
                    assert pred.dim() == 1
                    pending.append(writer.submit(audio_io.save_audio, out, pred[None, :].cpu().numpy(), self.sr))
                print(f"{os.path.basename(s)}, {os.path.basename(t)} -> {converted_audio_dir}")
            written = [f.result() for f in pending]
        finally:
            writer.shutdown(wait=True)
        return kdist.gather_paths(written)
