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

``f0_shift`` / ``transpose`` are kept as given (None included): serving.BatchConverter.pitch_of reads None as "this converter's
default".  No value changes an output's length or its file name, and with the defaults nothing changes at all.
Two constructors, one per calling convention: ``from_reference`` takes the upstream-named arguments of ``special_match``,
``bulk_match``, ``match_at_inference_time`` and the command line, where ``topk``, ``tgt_loudness_db`` and ``vad_trigger_level`` are
accepted and, as upstream, IGNORED unless their switch (``use_topk``, ``normalize_loudness``, ``use_vad``) is on; ``from_serving``
takes the "None = off" arguments of ``many_to_one``, ``TargetVoice`` and ``BatchConverter``.

What belongs to a *source item* (a request's own pitch values, its ``target_duration``, its blend weights) is NOT in this
record — the promise above about lengths holds because of that — but in ``SourceKnobs`` below, one per source.
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


@dataclass(frozen=True)
class SourceKnobs:
    """What one source item of a batch carries besides its audio; None: the converter's default, or off.  Built only by the
    converter's checks (serving.BatchConverter.pitch_of / duration_of / blend_of; RequestQueue.submit builds a request's at the
    door; match_at_inference_time copies the pitch values of its checked ``Extensions``), so holding one means the values are valid.

    ``target_duration`` (seconds) is a property of a source item, like a request's own ``transpose``: ``special_match``,
    ``many_to_one``, ``BatchConverter.convert`` and ``RequestQueue.submit`` take it as an argument of its own and hand it on in
    this record.  Its checks are ``matching.resolve_target_duration`` (the value) and ``matching.duration_plan`` (the ratio to
    the source's length).

    ``blend`` holds the weights of a voice blend (a conversion towards a weighted mix of 2 to 4 target voices; include/knnsvc_hip.h
    "Voice blend"), for the same reason: ``special_match`` / ``many_to_one`` take ``blend_with`` and ``blend``, ``BatchConverter``
    a sequence of ``TargetVoice`` and a default ``blend``, ``BatchConverter.convert`` and ``RequestQueue.submit`` a ``blend`` per
    source.  Its check is ``matching.resolve_blend``, which also normalises; every knob of ``Extensions`` acts on a blend as on a
    single target (the pitch knobs and ``topk`` inside every voice's match and in the one f0 shift, the tail on the blended
    frames)."""
    f0_shift: str | None = None
    transpose: float | None = None
    target_duration: float | None = None
    blend: tuple | None = None


def per_item(value, n, name, one=lambda v: v, default=None, is_list=None, unit="values"):
    """"A single value for all ``n`` items, or a list / tuple with one entry per item" -> a list of ``n`` entries, each
    ``one(entry)`` or, for a None entry, ``default``.  ``is_list``: for values that are sequences themselves (weight vectors),
    the predicate that tells a list of them from a single one.  ValueError (``name``, ``unit``) for a list of another length."""
    fill = lambda v: default if v is None else one(v)
    if not (is_list(value) if is_list is not None else isinstance(value, (list, tuple))):
        return [fill(value)] * n
    if len(value) != n:
        raise ValueError(f"{name}: {len(value)} {unit} for {n} items")
    return [fill(v) for v in value]
