"""``KNeighborsVC`` — the orchestrator object the reference's entry points hand out.

Mirror of ddsp_matcher.py:303-1155 restricted to its live methods: ``vocode``
(:375-406), ``special_match`` (:937-1023) and ``bulk_match`` (:1027-1155), with the
same argument names and output file naming.  ``topk`` is accepted and, as upstream, ignored UNLESS
``use_topk=True`` is passed (an extension, off by default): the match stage then mixes that many
(1..8) neighbours per frame instead of the hard-coded 4; file names do not change.
``tgt_loudness_db`` is accepted and, as in the reference's live methods, ignored UNLESS
``normalize_loudness=True`` is passed (an extension, off by default): the generator's waveform is
then brought to that integrated loudness on the GPU (ops.normalize_loudness; what the reference
documents for the argument, ddsp_matcher.py:533, 947, and does in its commented-out block
:997-1003).  ``audio_io.save_audio`` keeps the reference's peak rule — a waveform whose peak
exceeds 1 is divided by it — so a clip normalised past full scale is written lower than asked,
unless ``peak_db`` (below) holds its peaks under a ceiling first.  ``vad_trigger_level`` is accepted and, as in upstream's pool builder
(ddsp_prematch_dataset.py:1131 passes 7 to a function that drops it), ignored UNLESS ``use_vad=True``
is passed (an extension, off by default): silence is then trimmed from both ends of every TARGET
pool file on the GPU before it is encoded (ops.vad_trim: the sox `vad` effect with torchaudio's
default parameters as restated in include/knnsvc_hip.h; that restatement is the specification,
parity with torchaudio's own code is not pinned); the source is never trimmed, output length and
file names do not change.  ``f0_shift`` ("median", the default and upstream's; "octave", "semitone",
"none") and ``transpose`` (semitones, |t| <= 36, default 0) are an extension too: they choose how the
source's f0 is moved towards the target's (matching.F0_SHIFT_MODES; the interval is chosen per
utterance on the GPU) and take effect as passed; with the defaults nothing changes, and file names do
not change with any value.  ``envelope_mix`` (0..1, default 0 = off) and ``peak_db`` (dBFS <= 0, default
None = off) are an extension as well (output dynamics, csrc/dynamics.hip): the tail behind the generator then puts
the shape of the SOURCE's volume envelope back on the waveform (ops.envelope_mix: phrasing, fades and rests
survive; level-invariant), normalises the loudness when asked, and last holds the sample peaks under the
ceiling (ops.limit_peak), so that what is written respects it and ``save_audio``'s peak rule does not fire.
With the defaults nothing new is launched; file names do not change.  Other differences that are deliberate: ``special_match`` returns
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
from .matching import load_utterance, match_at_inference_time, resolve_dynamics, resolve_f0_shift
from .vocoder import Vocoder
from .wavlm import WavLMEncoder

# one-hot on layer 6 of 25 (ddsp_matcher.py:88-89, knnvc_utils.py:3-6)
SPEAKER_INFORMATION_WEIGHTS = [1.0 if i == C.MATCH_LAYER else 0.0 for i in range(25)]


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
        ``loudness_db`` (extension): every waveform is normalised to that integrated loudness before the finiteness check.
        ``envelope_mix`` / ``peak_db`` (extension, matching.resolve_dynamics): the source's envelope is mixed in before the
        loudness stage, the peak ceiling applied behind it.  ``src_wav``: the bs source waveforms (a [bs, L] tensor or a list of
        [L_b] tensors, 16 kHz mono as the encoder received them); needed when ``envelope_mix`` > 0."""
        a, p = resolve_dynamics(envelope_mix, peak_db)
        if a > 0.0 and src_wav is None:
            raise ValueError("vocode: envelope_mix > 0 needs src_wav, the source waveforms")
        if f0 is None:
            raise NotImplementedError("the f0-free 'wavlm_only_original' generator (hifigan/models.py) is missing "
                                      "from the reference snapshot and unsupported")
        outs = []
        for b in range(c.shape[0]):
            harm = harmonics_out_feats_weighted[b] if harmonics_out_feats_weighted is not None else None
            src = src_wav[b].reshape(-1).float().to(self.device) if a > 0.0 else None
            outs.append(self._vocode_async(c[b].to(self.device), f0[b].to(self.device), None if harm is None else harm.to(self.device),
                                           loudness_db=loudness_db, src_wav=src, envelope_mix=a, peak_db=p))
        wav = torch.stack(outs, 0)
        self._check_finite(wav)
        return wav

    @staticmethod
    def _check_finite(wav):
        # operand scales follow the data (range slots), so a non-finite sample means a non-finite input or weight
        if not bool(torch.isfinite(wav).all()):
            raise ops.KnnSvcError("vocode: non-finite waveform (non-finite features, f0, harmonics or weights)")

    def _vocode_async(self, c, f0, harm=None, loudness_db=None, src_wav=None, envelope_mix=0.0, peak_db=None):
        """One utterance, enqueue only (no host sync): the tail stage of the dataset-mode pipeline, in its fixed order:
        generator; envelope mix (``envelope_mix`` > 0: the shape of ``src_wav``'s envelope, first because it changes the level);
        loudness (``loudness_db``: measured and scaled to that level); peak ceiling (``peak_db``: last, so that what is written
        respects it).  All on the same stream, the first two in place (``Vocoder.forward`` hands out a copy)."""
        y = self.hifigan.forward(c.float(), f0.reshape(-1).float(), None if harm is None else harm.float())
        if envelope_mix:
            ops.envelope_mix(y, src_wav, envelope_mix, hop=self.hop_length, out=y)
        if loudness_db is not None:
            ops.normalize_loudness(y, loudness_db, self.sr, out=y)
        if peak_db is not None:
            y = ops.limit_peak(y, peak_db, self.sr)          # out of place: the parallel launch
        return y

    def _tail(self, f0only, loudness_db=None, envelope_mix=0.0, peak_db=None):
        """``vocode_fn`` of the stream pipeline: generator, then the stages asked for (``_vocode_async``).  With the envelope mix
        it is the four-argument form ``(out_feats, shifted_f0, harm, src_wav)``, else the three-argument one."""
        kw = dict(loudness_db=loudness_db, peak_db=peak_db)
        if envelope_mix:
            kw["envelope_mix"] = envelope_mix
            if f0only:
                return lambda c, f0, _h, src: self._vocode_async(c, f0, src_wav=src, **kw)
            return lambda c, f0, h, src: self._vocode_async(c, f0, h, src_wav=src, **kw)
        if f0only:
            return lambda c, f0, _h: self._vocode_async(c, f0, **kw)
        return lambda c, f0, h: self._vocode_async(c, f0, h, **kw)

    @torch.inference_mode()
    def special_match(self, src_wav_file, ref_wav_file, topk: int = 4, device=None, prioritize_f0=True,
                      ckpt_type="wavlm_only", tgt_loudness_db=-16, post_opt="no_post_opt", save=True, normalize_loudness=False,
                      use_topk=False, use_vad=False, vad_trigger_level=7, f0_shift="median", transpose=0.0, envelope_mix=0.0,
                      peak_db=None):
        level = tgt_loudness_db if normalize_loudness else None
        resolve_f0_shift(f0_shift, transpose)            # refused before a file is read
        mix, ceiling = resolve_dynamics(envelope_mix, peak_db)      # likewise
        dyn = lambda: dict(src_wav=[torch.from_numpy(load_utterance(src_wav_file)[0])] if mix > 0.0 else None, envelope_mix=mix,
                           peak_db=ceiling)
        f0only = "wavlm_only" in ckpt_type or "no_harm_no_amp" in ckpt_type
        if "wavlm_only_original" in ckpt_type:
            raise NotImplementedError("wavlm_only_original needs hifigan/models.py, absent upstream")
        key = str(src_wav_file)
        if not f0only:
            of, hw, _a, sf0 = match_at_inference_time(Path(src_wav_file), Path(ref_wav_file), self.wavlm,
                                                      self.weighting, self.weighting, topk=topk, device=self.device,
                                                      prioritize_f0=prioritize_f0, ckpt_type=ckpt_type, post_opt=post_opt,
                                                      use_topk=use_topk, use_vad=use_vad, vad_trigger_level=vad_trigger_level,
                                                      f0_shift=f0_shift, transpose=transpose)
            pred = self.vocode(of[key][None], sf0[key][None, :, None], hw[key][None], loudness_db=level, **dyn()).squeeze()
        else:
            # the reference does not forward post_opt on this branch (ddsp_matcher.py:970)
            of, _a, sf0 = match_at_inference_time(Path(src_wav_file), Path(ref_wav_file), self.wavlm,
                                                  self.weighting, self.weighting, topk=topk, device=self.device,
                                                  prioritize_f0=prioritize_f0, ckpt_type=ckpt_type, use_topk=use_topk,
                                                  use_vad=use_vad, vad_trigger_level=vad_trigger_level,
                                                  f0_shift=f0_shift, transpose=transpose)
            pred = self.vocode(of[key][None], sf0[key][None, :, None], loudness_db=level, **dyn()).squeeze()
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
                    f0_shift=None, transpose=None, envelope_mix=None, peak_db=None):
        """BASELINE cfg 5 (no counterpart upstream: the reference would call ``special_match`` once per source and rebuild the
        target pool each time, ddsp_matcher.py:937-1023): MANY sources against ONE target pool that is built once and stays
        resident, all sources through the stream pipeline as one batch (knn_svc_amd/serving.py).  Under a process group the
        sources are dealt over the ranks (no collective).  ``target``: a serving.TargetVoice to reuse.  -> written paths (all
        ranks' on every rank), named like ``special_match``'s outputs.  ``match``: "lanes" | "segmented" (serving.BatchConverter; default
        from KNNSVC_MATCH).  ``loudness_db``: every waveform is normalised to that integrated loudness (None: left as generated).
        ``topk``: neighbours mixed per frame, 1..8 (None: 4).  ``vad_trigger_level``: the pool's files are trimmed of the silence
        at both ends with that trigger level (None: left whole; ignored when ``target`` is given).  ``f0_shift`` / ``transpose``:
        the f0 shift mode and the transpose in semitones of every source (None: "median" / 0).  ``envelope_mix`` / ``peak_db``: how
        much of each source's volume envelope is put back on its output (0..1) and the sample-peak ceiling in dBFS (None: off)."""
        from . import serving
        resolve_f0_shift(f0_shift, transpose)            # refused before a file is read
        resolve_dynamics(envelope_mix, peak_db)
        if target is None:
            target = serving.TargetVoice(self, ref_wav_file, duration_limit, vad_trigger_level=vad_trigger_level)
        mine = kdist.my_share([str(p) for p in src_files])
        written = serving.BatchConverter(self, target, ckpt_type, post_opt, match=match,
                                         loudness_db=loudness_db, topk=topk, f0_shift=f0_shift,
                                         transpose=transpose, envelope_mix=envelope_mix, peak_db=peak_db).convert_files(mine, converted_audio_dir)
        return kdist.gather_paths(written)

    @torch.inference_mode()
    def bulk_match(self, src_dataset_path, tgt_dataset_path, converted_audio_dir, topk: int = 4, device=None,
                   prioritize_f0=True, ckpt_type="mix", tgt_loudness_db=-16, required_subset_file=None,
                   post_opt="no_post_opt", duration_limit=None, normalize_loudness=False, use_topk=False, use_vad=False,
                   vad_trigger_level=7, f0_shift="median", transpose=0.0, envelope_mix=0.0, peak_db=None):
        level = tgt_loudness_db if normalize_loudness else None
        resolve_f0_shift(f0_shift, transpose)            # refused before a file is read
        mix, ceiling = resolve_dynamics(envelope_mix, peak_db)      # likewise
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
                common = dict(topk=topk, device=self.device, prioritize_f0=prioritize_f0, ckpt_type=ckpt_type,
                              src_dataset_path=src_dataset_path, tgt_dataset_path=tgt_dataset_path,
                              required_subset=required, duration_limit=duration_limit,
                              pool_sharded=shard, share_items=shard, use_topk=use_topk, use_vad=use_vad,
                              vad_trigger_level=vad_trigger_level, f0_shift=f0_shift, transpose=transpose)
                # the generator of every utterance is the tail stage of the match pipeline (same kernels and inputs as
                # `vocode` after the fact, ddsp_matcher.py:1114-1128, but enqueued under the next utterances' matching);
                # one finiteness check per speaker pair instead of one host sync per utterance; with normalize_loudness,
                # envelope_mix or peak_db the tail is generator + those stages, still enqueue-only
                preds = {}
                if not f0only:
                    match_at_inference_time(Path(s), Path(t), self.wavlm, self.weighting, self.weighting, post_opt=post_opt,
                                            vocode_fn=self._tail(False, level, mix, ceiling), waves_out=preds, **common)
                else:
                    match_at_inference_time(Path(s), Path(t), self.wavlm, self.weighting, self.weighting,
                                            vocode_fn=self._tail(True, level, mix, ceiling), waves_out=preds, **common)
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
