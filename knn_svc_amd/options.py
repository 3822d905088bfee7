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

Harmony parts (``Harmony`` / ``HarmonyPart`` below; include/knnsvc_hip.h "Harmony voice") belong to a source item too, but they are
not a field of ``SourceKnobs``: a source with P parts becomes 1 + P items of the match stage that share its knobs, and what tells
a part from its lead, the ``HarmonyShift`` (mask, steps, alpha, log_ref), travels in a record of its own beside the item's knobs
(matching.match_bodies ``parts=``; the match functions' ``harmony=``).

  argument       off (default)       on                                                                    where it acts
  harmony        None                an options.Harmony: 1..3 parts, each the lead's final f0 moved by      match stage, behind the
                                     scale degrees with the lead's deviation kept, matched as an item of    correction (ops.harmony_f0_seg);
                                     its own from the lead's encoder output and neighbour list, and mixed   tail, between its per-voice and
                                     under the lead on the GPU                                              per-output halves (ops.mix_waves)
"""
from __future__ import annotations

import math
import numbers
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


TUNE_TONICS = {"c": 0, "c#": 1, "db": 1, "d": 2, "d#": 3, "eb": 3, "e": 4, "f": 5, "f#": 6, "gb": 6, "g": 7, "g#": 8, "ab": 8,
               "a": 9, "a#": 10, "bb": 10, "b": 11}
# scale name -> the twelve pitch classes from the tonic upwards, '1' = allowed
TUNE_SCALES = {"major": "101011010101", "minor": "101101011010", "harmonic_minor": "101101011001", "pentatonic": "101010010100",
               "minor_pentatonic": "100101010010", "blues": "100101110010"}
TUNE_FRAME_MS = 20.0          # the frame period of the f0 track (hop 320 at 16 kHz)


def scale_mask(scale) -> int:
    """A scale as the library's 12-bit mask (bit k: pitch class k is allowed, C = 0).  Case-insensitive: ``"chromatic"``,
    ``"<tonic>:<name>"`` (TUNE_TONICS, TUNE_SCALES) or ``"<tonic>:<twelve 0/1 characters>"``, the first of them the tonic, the
    pattern rotated by the tonic into the C-based mask.  ValueError for anything else, a pattern without a 1 included."""
    if not isinstance(scale, str):
        raise ValueError(f"tune: a scale is a string such as 'chromatic', 'A:minor' or 'D:101011010101', got {scale!r}")
    text = scale.strip().lower()
    if text == "chromatic":
        return 0xFFF
    tonic, sep, name = text.partition(":")
    if not sep or tonic not in TUNE_TONICS:
        raise ValueError(f"tune: scale {scale!r} is neither 'chromatic' nor '<tonic>:<name or twelve 0/1>' with a tonic out of "
                         f"{' '.join(t.capitalize() for t in TUNE_TONICS)}")
    pattern = TUNE_SCALES.get(name, name)
    if len(pattern) != 12 or set(pattern) - {"0", "1"}:
        raise ValueError(f"tune: scale {scale!r}: {name!r} is neither one of {tuple(TUNE_SCALES)} nor twelve 0/1 characters")
    if "1" not in pattern:
        raise ValueError(f"tune: scale {scale!r} allows no pitch class")
    mask = 0
    for j, ch in enumerate(pattern):
        if ch == "1":
            mask |= 1 << ((TUNE_TONICS[tonic] + j) % 12)
    return mask


def _number(value, name, lo, hi):
    """``value`` as a float in [lo, hi]; no bools or strings where numbers go."""
    if isinstance(value, bool) or not isinstance(value, numbers.Real) or not lo <= float(value) <= hi:      # (NaN compares false)
        raise ValueError(f"tune: {name} must be a number in [{lo:g}, {hi:g}], got {value!r}")
    return float(value)


@dataclass(frozen=True)
class Tuning:
    """Pitch correction of one source item (include/knnsvc_hip.h "Pitch correction" is the specification): the key and scale the
    OUTPUT is snapped towards, how far (``strength`` in [0, 1]; 0: off), how fast (``retune_ms`` in [0, 2000]: the time constant
    of the glide onto a note; 0: a hard snap that also removes vibrato, 80 and more leave vibrato alone) and the frequency of
    A4 (``tuning_hz`` in [400, 480]).  Checked on construction, so holding one means the values are valid.  ``mask``, ``alpha`` and
    ``log_ref`` are what the library takes."""
    scale: str
    strength: float = 1.0
    retune_ms: float = 80.0
    tuning_hz: float = 440.0

    def __post_init__(self):
        scale_mask(self.scale)
        for name, lo, hi in (("strength", 0.0, 1.0), ("retune_ms", 0.0, 2000.0), ("tuning_hz", 400.0, 480.0)):
            object.__setattr__(self, name, _number(getattr(self, name), name, lo, hi))

    @property
    def mask(self) -> int:
        return scale_mask(self.scale)

    @property
    def alpha(self) -> float:
        return 1.0 if self.retune_ms == 0 else -math.expm1(-TUNE_FRAME_MS / self.retune_ms)

    @property
    def log_ref(self) -> float:
        return math.log(self.tuning_hz)

    @property
    def on(self) -> bool:
        return self.strength > 0


TUNE_OFF = Tuning("chromatic", strength=0.0)      # "off" for an item under a converter whose default is on


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
    frames).

    ``tune`` holds the pitch correction (a ``Tuning``; None: the converter's default, or off): a key belongs to a song, that is,
    to a source item.  ``special_match``, ``bulk_match``, ``many_to_one`` and ``match_at_inference_time`` take ``tune=``,
    ``BatchConverter(tune=)`` holds the default beside its default blend, ``BatchConverter.convert`` and ``RequestQueue.submit``
    take one per source ("off" switches a default off).  Its check is ``matching.resolve_tune``.

      field          off (default)       on                                                                    where it acts
      tune           None                a Tuning, or its scale as a string ("chromatic", "A:minor",           match stage, behind the f0
                                         "D:101011010101"): the shifted f0 is snapped towards the notes of     shift (ops.tune_f0_seg)
                                         that key on the GPU; f0 re-rank, pitched re-selection and vocoder
                                         all see the corrected contour
    The key is the key of the OUTPUT: correction follows the shift, ``transpose``, a blend's one shift and
    ``target_duration``'s re-timing, so ``retune_ms`` runs in output time.  With ``f0_shift="median"`` the interval is an
    arbitrary real number and correction is what puts the result on a grid; with "semitone" / "octave" / "none" plus a whole
    ``transpose`` the output's key is the source's key moved by that interval."""
    f0_shift: str | None = None
    transpose: float | None = None
    target_duration: float | None = None
    blend: tuple | None = None
    tune: Tuning | None = None


HARMONY_MAX_PARTS = 3        # KNNSVC_HARMONY_MAX_PARTS
HARMONY_MAX_STEPS = 24       # KNNSVC_HARMONY_MAX_STEPS


def _harmony_number(value, name, lo, hi):
    if isinstance(value, bool) or not isinstance(value, numbers.Real) or not lo <= float(value) <= hi:      # (NaN compares false)
        raise ValueError(f"harmony: {name} must be a number in [{lo:g}, {hi:g}], got {value!r}")
    return float(value)


@dataclass(frozen=True)
class HarmonyPart:
    """One harmony part: ``steps`` scale degrees above (> 0) or below (< 0) the lead, a non-zero int in -24..24 (2: a third
    above, -5: a sixth below, +-7 in a seven-note scale: an octave), and its level in the mix, ``gain_db`` in [-60, 12].
    Checked on construction."""
    steps: int
    gain_db: float = -6.0

    def __post_init__(self):
        s = self.steps
        if isinstance(s, bool) or not isinstance(s, numbers.Integral) or int(s) == 0 or abs(int(s)) > HARMONY_MAX_STEPS:
            raise ValueError(f"harmony: steps must be a non-zero int in -{HARMONY_MAX_STEPS}..{HARMONY_MAX_STEPS} (scale degrees), got {s!r}")
        object.__setattr__(self, "steps", int(s))
        object.__setattr__(self, "gain_db", _harmony_number(self.gain_db, "gain_db", -60.0, 12.0))

    @property
    def gain(self) -> float:
        return 10.0 ** (self.gain_db / 20.0)


@dataclass(frozen=True)
class HarmonyShift:
    """What the library takes for one part (include/knnsvc_hip.h "Harmony voice"): ``(mask, steps, alpha, log_ref)``.  It travels
    in a record of its own beside the item's ``SourceKnobs``; built only by ``Harmony.shifts``, so holding one means the values
    are valid."""
    mask: int
    steps: int
    alpha: float
    log_ref: float

    @property
    def on(self) -> bool:
        return self.mask != 0 and self.steps != 0


@dataclass(frozen=True)
class Harmony:
    """Harmony parts of one source item (include/knnsvc_hip.h "Harmony voice" is the specification): 1 to 3 ``parts``
    (``HarmonyPart``, or bare ints for their steps), each the lead's contour moved by scale degrees in ``scale``, sung by the
    same target voice and mixed under the lead on the GPU.  Checked on construction.

      field       default             meaning
      parts       (required)          1..3 HarmonyPart or ints: degrees above / below the lead, each with its gain_db (-6)
      scale       None: the item's    the key the parts move in ("chromatic": parallel parts of ``steps`` semitones; "A:minor";
                  ``tune`` scale      "D:101011010101"); without a scale here and without a ``tune`` on the item: ValueError
      lead_db     0.0                 the lead's level in the mix, [-60, 12] dB
      glide_ms    40.0                [0, 2000]: where the lead changes note a part's interval changes too; the time constant of
                                      that change (0: a jump), a = -expm1(-20 / glide_ms)
      tuning_hz   None: the item's    the frequency of A4, [400, 480]; None without a ``tune``: 440
                  ``tune`` tuning
    A different target voice per part and stems from the command line are out of scope."""
    parts: tuple
    scale: str | None = None
    lead_db: float = 0.0
    glide_ms: float = 40.0
    tuning_hz: float | None = None

    def __post_init__(self):
        parts = self.parts
        if isinstance(parts, (HarmonyPart, numbers.Integral)) and not isinstance(parts, bool):
            parts = (parts,)
        if isinstance(parts, (str, bytes)) or not isinstance(parts, (list, tuple)):
            raise ValueError(f"harmony: parts must be a sequence of 1..{HARMONY_MAX_PARTS} HarmonyPart or ints, got {self.parts!r}")
        if not 1 <= len(parts) <= HARMONY_MAX_PARTS:
            raise ValueError(f"harmony: {len(parts)} parts, expected 1..{HARMONY_MAX_PARTS}")
        object.__setattr__(self, "parts", tuple(p if isinstance(p, HarmonyPart) else HarmonyPart(p) for p in parts))
        if self.scale is not None:
            scale_mask_for_harmony(self.scale)
        object.__setattr__(self, "lead_db", _harmony_number(self.lead_db, "lead_db", -60.0, 12.0))
        object.__setattr__(self, "glide_ms", _harmony_number(self.glide_ms, "glide_ms", 0.0, 2000.0))
        if self.tuning_hz is not None:
            object.__setattr__(self, "tuning_hz", _harmony_number(self.tuning_hz, "tuning_hz", 400.0, 480.0))

    @property
    def alpha(self) -> float:
        return 1.0 if self.glide_ms == 0 else -math.expm1(-TUNE_FRAME_MS / self.glide_ms)

    @property
    def gains(self) -> tuple:
        """The linear gains of the mix, lead first."""
        return (10.0 ** (self.lead_db / 20.0),) + tuple(p.gain for p in self.parts)

    def shifts(self, tune=None) -> tuple:
        """-> one ``HarmonyShift`` per part, with the scale and tuning frequency taken from ``tune`` (the item's Tuning; one that
        is off counts as none) where this record leaves them open.  ValueError without a scale."""
        tune = tune if tune is not None and tune.on else None
        scale = self.scale if self.scale is not None else (tune.scale if tune is not None else None)
        if scale is None:
            raise ValueError("harmony: no scale: give Harmony(scale=...) or a tune= with the key of the song")
        hz = self.tuning_hz if self.tuning_hz is not None else (tune.tuning_hz if tune is not None else 440.0)
        mask, a, lr = scale_mask_for_harmony(scale), self.alpha, math.log(hz)
        return tuple(HarmonyShift(mask, p.steps, a, lr) for p in self.parts)


def scale_mask_for_harmony(scale) -> int:
    """``scale_mask`` with the message of a harmony."""
    try:
        return scale_mask(scale)
    except ValueError as e:
        raise ValueError(str(e).replace("tune:", "harmony:", 1)) from None


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
