"""The extension knobs of a conversion as ONE checked value.  Every entry point builds an ``Extensions`` as its first statement
(a bad value is refused before a file is read or a model is used) and hands the record on; holding one means the values are valid.

  field          off (default)       on                                                                    where it acts
  topk           None: 4, upstream   1..8 neighbours mixed per frame out of the 32 found                   match stage
  vad_level      0: pool left whole  > 1e-3: silence trimmed from both ends of every TARGET pool file on   get_complete_spk_pool
                                     the GPU before it is encoded (ops.vad_trim: the sox `vad` effect as
                                     restated in include/knnsvc_hip.h — that restatement is the
                                     specification); the source is never trimmed
  f0_shift       None: "median"      "median" | "octave" | "semitone" | "none" (matching.F0_SHIFT_MODES):  match stage (f0 shift)
                                     how the source's f0 is moved towards the target's; the interval is
                                     chosen per utterance on the GPU
  transpose      None: 0             semitones on top in every mode, |t| <= 36                             match stage (f0 shift)
  envelope_mix   0.0                 (0, 1]: that much of the SHAPE of the source's volume envelope put    tail, 1st (ops.envelope_mix)
                                     back on the waveform (phrasing, fades, rests; level-invariant)
  loudness_db    None                the waveform brought to that integrated loudness (BS.1770)            tail, 2nd (ops.normalize_loudness)
  peak_db        None                dBFS <= 0: sample peaks held under that ceiling, so that what is      tail, 3rd (ops.limit_peak)
                                     written respects it and save_audio's peak rule does not fire

``f0_shift`` / ``transpose`` are kept as given (None included): serving.BatchConverter.pitch_of and RequestQueue read None as
"this converter's default".  No value changes an output's length or its file name, and with the defaults nothing changes at all.
Two constructors, one per calling convention: ``from_reference`` takes the upstream-named arguments of ``special_match``,
``bulk_match``, ``match_at_inference_time`` and the command line, where ``topk``, ``tgt_loudness_db`` and ``vad_trigger_level`` are
accepted and, as upstream, IGNORED unless their switch (``use_topk``, ``normalize_loudness``, ``use_vad``) is on; ``from_serving``
takes the "None = off" arguments of ``many_to_one``, ``TargetVoice`` and ``BatchConverter``.

``target_duration`` is NOT a field of this record, and the promise above about lengths holds because of that: a duration is a
property of a *source item*, like a request's own ``transpose``, and travels beside the record (``special_match``,
``many_to_one``, ``BatchConverter.convert`` and ``RequestQueue.submit`` take it as an argument of its own).  Its checks are
``matching.resolve_target_duration`` (the value) and ``matching.duration_plan`` (the ratio to the source's length).

The weights of a voice blend (``blend``: a conversion towards a weighted mix of 2 to 4 target voices; include/knnsvc_hip.h "Voice
blend") are NOT a field either, for the same reason: a weight vector is a property of a source item and travels beside the record
(``special_match`` / ``many_to_one`` take ``blend_with`` and ``blend``, ``BatchConverter`` a sequence of ``TargetVoice`` and a
default ``blend``, ``BatchConverter.convert`` and ``RequestQueue.submit`` a ``blend`` per source).  Its check is
``matching.resolve_blend``, which also normalises; every knob of the record acts on a blend as on a single target (the pitch knobs
and ``topk`` inside every voice's match and in the one f0 shift, the tail on the blended frames).
"""
from __future__ import annotations

from dataclasses import dataclass


@dataclass(frozen=True)
class Extensions:
    topk: int | None = None
    vad_level: float = 0
    f0_shift: str | None = None
    transpose: float | None = None
    loudness_db: float | None = None
    envelope_mix: float = 0.0
    peak_db: float | None = None

    @classmethod
    def from_serving(cls, loudness_db=None, topk=None, vad_trigger_level=None, f0_shift=None, transpose=None, envelope_mix=None,
                     peak_db=None):
        from .matching import resolve_dynamics, resolve_f0_shift, resolve_topk      # (matching builds records itself)
        resolve_f0_shift(f0_shift, transpose)
        mix, ceiling = resolve_dynamics(envelope_mix, peak_db)
        return cls(topk=None if topk is None else resolve_topk(topk), vad_level=0 if vad_trigger_level is None else vad_trigger_level,
                   f0_shift=f0_shift, transpose=transpose, loudness_db=None if loudness_db is None else float(loudness_db),
                   envelope_mix=mix, peak_db=ceiling)

    @classmethod
    def from_reference(cls, topk=4, use_topk=False, tgt_loudness_db=-16, normalize_loudness=False, use_vad=False,
                       vad_trigger_level=7, f0_shift="median", transpose=0.0, envelope_mix=0.0, peak_db=None):
        return cls.from_serving(loudness_db=tgt_loudness_db if normalize_loudness else None, topk=topk if use_topk else None,
                                vad_trigger_level=vad_trigger_level if use_vad else None, f0_shift=f0_shift, transpose=transpose,
                                envelope_mix=envelope_mix, peak_db=peak_db)
