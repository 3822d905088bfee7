"""Command line front end with the flags of the reference's ``ddsp_inference.py`` (:27-46).

  python ddsp_inference.py SRC TGT [--ckpt_dir D] [--ckpt_type mix] [--post_opt post_opt_0.2] ...

SRC/TGT are both audio files (single conversion, output next to SRC as
``<src>_to_<tgt>_knn_<ckpt_type>_<post_opt>.wav``) or both dataset roots (folders of
speaker folders; outputs under ``<tgt parent>/<src>_to_<tgt>_<ckpt_type>_post_opt_<post_opt>/``,
prefixed ``duration_limit_<n>_`` when --dur_limit is given).  --topk / --use_topk,
--tgt_loudness_db / --normalize_loudness, --vad_trigger_level / --use_vad, --f0_shift,
--transpose, --envelope_mix and --peak_db are the extension knobs (knn_svc_amd/options.py has
the table; the first three values are accepted and, as upstream, ignored unless their switch
is true); no value changes a file name, and a clip normalised past full scale is written
lower than asked (save_audio divides by a peak above 1, as upstream) unless --peak_db holds
its peaks under a ceiling (where the limiter engages the loudness ends below the target).  --target_duration
SECONDS (file mode only; upstream documents the argument and never delivers it) re-times the conversion to
that length (matching.duration_plan; the file name does not change).  --blend_tgt PATH (file mode only, up to
three times) adds target voices and --blend W0,W1[,...] weighs TGT and them: the conversion goes towards that mix
(matcher.KNeighborsVC.blend_voices; the output is named <src>_to_<tgt>+<blend_tgt>..., without the weights).  --tune SCALE
("chromatic", "A:minor", "D:101011010101"; options.Tuning) snaps the converted f0 towards the notes of that key — the key of the
OUTPUT —, with --tune_strength S (0..1), --retune_ms MS (0..2000; 0: hard snap) and --tuning_hz HZ (400..480) as its
refinements, refused without --tune; no file name changes.  --harmony_steps 2,-3 (file mode only; options.Harmony) adds
harmony parts, each the lead's contour moved by that many scale degrees, sung by the same target voice and mixed under the lead:
--harmony_scale S (default: --tune's scale), --harmony_gain_db -6,-9 (one per part, default -6), --harmony_lead_db 0 and
--harmony_glide_ms 40 refine it and are refused without --harmony_steps; the mix is written, no file name changes (stems and a
different target voice per part are not offered).  --dur_limit is
compared in seconds, as upstream (ddsp_prematch_dataset.py:408-411).
"""
from __future__ import annotations

import argparse
import os
import re

FLAGS = [
    ("--ckpt_dir", dict(type=str, default="/home/ken/Downloads/knn_vc_data/ckpt_saved")),
    ("--ckpt_type", dict(type=str, default="mix")),
    ("--post_opt", dict(type=str, default="no_post_opt")),
    ("--required_subset_file", dict(type=str, default=None)),
    ("--topk", dict(type=int, default=4)),
    ("--device", dict(type=str, default="cuda")),
    ("--tgt_loudness_db", dict(type=float, default=-16)),
    ("--dur_limit", dict(type=int, default=None)),
]


def _bool(v: str) -> bool:
    v = v.lower()
    if v in ("yes", "true", "t", "1", "y"):
        return True
    if v in ("no", "false", "f", "0", "n"):
        return False
    raise argparse.ArgumentTypeError("boolean value expected")


def _steps(v: str) -> list:
    try:
        return [int(w) for w in v.split(",")]
    except ValueError:
        raise argparse.ArgumentTypeError("comma-separated whole numbers expected, e.g. 2,-3")


def _weights(v: str) -> list:
    try:
        return [float(w) for w in v.split(",")]
    except ValueError:
        raise argparse.ArgumentTypeError("comma-separated numbers expected, e.g. 0.7,0.3")


def build_parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(description="kNN-SVC inference (MI355X build): file or folder mode")
    # a comma-separated list that starts with a negative number ("--harmony_gain_db -6,-9") is a value, not an option
    ap._negative_number_matcher = re.compile(r"^-\d[\d.,eE+-]*$|^-\.\d[\d.,eE+-]*$")
    ap.add_argument("src")
    ap.add_argument("tgt")
    for flag, kw in FLAGS:
        ap.add_argument(flag, **kw)
    ap.add_argument("--prioritize_f0", type=_bool, default=True)
    ap.add_argument("--normalize_loudness", type=_bool, default=False,
                    help="(extension) normalise every output to --tgt_loudness_db LKFS")
    ap.add_argument("--use_topk", type=_bool, default=False,
                    help="(extension) mix --topk (1..8) neighbours per frame instead of the reference's hard-coded 4")
    ap.add_argument("--use_vad", type=_bool, default=False,
                    help="(extension) trim silence from both ends of every target pool file (--vad_trigger_level)")
    ap.add_argument("--vad_trigger_level", type=float, default=7,
                    help="(extension, with --use_vad true) trigger level of the trimmer; higher keeps less")
    ap.add_argument("--f0_shift", type=str, default="median", choices=["median", "octave", "semitone", "none"],
                    help="(extension) how the source's f0 is moved towards the target's: by the difference of the medians, "
                         "by that difference rounded to octaves or semitones, or not at all")
    ap.add_argument("--transpose", type=float, default=0.0,
                    help="(extension) semitones added to the f0 shift in every mode, at most 36 either way")
    ap.add_argument("--envelope_mix", type=float, default=0.0,
                    help="(extension) 0..1: how much of the source's volume envelope is put back on the output (0 = off)")
    ap.add_argument("--peak_db", type=float, default=None,
                    help="(extension) sample-peak ceiling of the output in dBFS, <= 0 (default: none)")
    ap.add_argument("--target_duration", type=float, default=None, metavar="SECONDS",
                    help="(extension, file mode only) re-time the conversion to this length; between a quarter of and four "
                         "times the source's; not together with --envelope_mix")
    ap.add_argument("--blend_tgt", action="append", default=None, metavar="PATH",
                    help="(extension, file mode only; up to three times) a further target voice: the conversion goes towards a "
                         "weighted mix of TGT and these")
    ap.add_argument("--blend", type=_weights, default=None, metavar="W0,W1[,...]",
                    help="(extension, with --blend_tgt) the weights of TGT and of each --blend_tgt in order; normalised to sum "
                         "1 (default: equal)")
    ap.add_argument("--tune", type=str, default=None, metavar="SCALE",
                    help="(extension) pitch correction: snap the converted f0 towards the notes of this key, the key of the output: "
                         "'chromatic', '<tonic>:<major|minor|harmonic_minor|pentatonic|minor_pentatonic|blues>' or "
                         "'<tonic>:<twelve 0/1 from the tonic>'")
    ap.add_argument("--tune_strength", type=float, default=None, metavar="S", help="(extension, with --tune) 0..1, default 1")
    ap.add_argument("--retune_ms", type=float, default=None, metavar="MS",
                    help="(extension, with --tune) time constant of the glide onto a note, 0..2000, default 80; 0 is a hard snap")
    ap.add_argument("--tuning_hz", type=float, default=None, metavar="HZ",
                    help="(extension, with --tune) the frequency of A4, 400..480, default 440")
    ap.add_argument("--harmony_steps", type=_steps, default=None, metavar="N[,N[,N]]",
                    help="(extension, file mode only) one to three harmony parts, each that many scale degrees above (> 0) or below "
                         "(< 0) the lead, e.g. 2,-3: a third above and a fourth below")
    ap.add_argument("--harmony_scale", type=str, default=None, metavar="S",
                    help="(extension, with --harmony_steps) the key the parts move in, as --tune takes it; default: --tune's scale")
    ap.add_argument("--harmony_gain_db", type=_weights, default=None, metavar="DB[,DB[,DB]]",
                    help="(extension, with --harmony_steps) the level of each part in the mix, -60..12, default -6")
    ap.add_argument("--harmony_lead_db", type=float, default=None, metavar="DB",
                    help="(extension, with --harmony_steps) the level of the lead in the mix, -60..12, default 0")
    ap.add_argument("--harmony_glide_ms", type=float, default=None, metavar="MS",
                    help="(extension, with --harmony_steps) how fast a part's interval changes where the lead changes note, "
                         "0..2000, default 40; 0 is a jump")
    ap.add_argument("--weights", default="auto", choices=["auto", "checkpoint", "seeded"],
                    help="(extension) 'seeded' runs with random weights when the released checkpoints are unavailable")
    return ap


def output_dir_for(src: str, tgt: str, ckpt_type: str, post_opt: str, dur_limit) -> str:
    parent = f"{os.path.dirname(os.path.abspath(tgt))}/"
    out = f"{parent}{os.path.basename(src)}_to_{os.path.basename(tgt)}_{ckpt_type}_post_opt_{post_opt}/"
    if dur_limit is not None:
        out = out.replace(parent, parent + f"duration_limit_{dur_limit}_")
    return out


def tuning_of(a):
    """The command line's --tune flags as an options.Tuning (None without --tune); ValueError for a bad value or a refinement
    without --tune."""
    from .options import Tuning
    more = {k: v for k, v in (("strength", a.tune_strength), ("retune_ms", a.retune_ms), ("tuning_hz", a.tuning_hz)) if v is not None}
    if a.tune is None:
        if more:
            raise ValueError("--tune_strength / --retune_ms / --tuning_hz refine --tune SCALE: give a scale")
        return None
    return Tuning(scale=a.tune, **more)


def harmony_of_flags(a, tune=None):
    """The command line's --harmony flags as an options.Harmony (None without --harmony_steps), checked against ``tune`` (the
    --tune flags' Tuning): ValueError for a bad value, a refinement without --harmony_steps, gains that are not one per part, or
    no scale in either."""
    from .options import Harmony, HarmonyPart
    more = {k: v for k, v in (("scale", a.harmony_scale), ("lead_db", a.harmony_lead_db), ("glide_ms", a.harmony_glide_ms)) if v is not None}
    if a.harmony_steps is None:
        if more or a.harmony_gain_db is not None:
            raise ValueError("--harmony_scale / --harmony_gain_db / --harmony_lead_db / --harmony_glide_ms refine --harmony_steps: give the steps")
        return None
    gains = a.harmony_gain_db if a.harmony_gain_db is not None else [-6.0] * len(a.harmony_steps)
    if len(gains) != len(a.harmony_steps):
        raise ValueError(f"--harmony_gain_db: {len(gains)} gains for {len(a.harmony_steps)} parts")
    h = Harmony(tuple(HarmonyPart(s, g) for s, g in zip(a.harmony_steps, gains)), **more)
    h.shifts(tune)
    return h


def main(argv=None) -> int:
    ap = build_parser()
    a = ap.parse_args(argv)
    from .options import Extensions
    knobs = dict(topk=a.topk, use_topk=a.use_topk, tgt_loudness_db=a.tgt_loudness_db, normalize_loudness=a.normalize_loudness,
                 use_vad=a.use_vad, vad_trigger_level=a.vad_trigger_level, f0_shift=a.f0_shift, transpose=a.transpose,
                 envelope_mix=a.envelope_mix, peak_db=a.peak_db)
    try:
        ext = Extensions.from_reference(**knobs)           # before the models are loaded
        from .matching import refuse_duration_with_envelope, resolve_target_duration
        refuse_duration_with_envelope([resolve_target_duration(a.target_duration)], ext)
        tune = tuning_of(a)
        harmony = harmony_of_flags(a, tune)
    except ValueError as e:
        ap.error(str(e))
    if harmony is not None and os.path.isdir(a.src):
        ap.error("--harmony_steps applies to a single conversion: a dataset run returns one feature set per utterance")
    if (a.blend_tgt is not None or a.blend is not None) and os.path.isdir(a.src):
        ap.error("--blend_tgt / --blend apply to a single conversion: a dataset run pairs speakers, a blend has no meaning there")
    try:                                                   # the count of voices and of weights, before the models are loaded
        from .matcher import KNeighborsVC
        KNeighborsVC.blend_voices(a.tgt, a.blend_tgt, a.blend)
    except ValueError as e:
        ap.error(str(e))
    if a.target_duration is not None and os.path.isdir(a.src):
        ap.error("--target_duration applies to a single source file: one duration for a dataset of utterances means nothing")
    from .hubconf import knn_vc
    knn = knn_vc(pretrained=True, progress=True, prematched=True, device=a.device, ckpt_type=a.ckpt_type,
                 local_ckpt_dir=a.ckpt_dir, weights=a.weights)
    common = dict(device=a.device, prioritize_f0=a.prioritize_f0, ckpt_type=a.ckpt_type, post_opt=a.post_opt, **knobs,
                  **({} if tune is None else dict(tune=tune)))
    if os.path.isfile(a.src) and os.path.isfile(a.tgt):
        knn.special_match(src_wav_file=a.src, ref_wav_file=a.tgt, target_duration=a.target_duration, blend_with=a.blend_tgt,
                          blend=a.blend, **({} if harmony is None else dict(harmony=harmony)), **common)
        return 0
    if os.path.isdir(a.src) and os.path.isdir(a.tgt):
        knn.bulk_match(src_dataset_path=a.src, tgt_dataset_path=a.tgt,
                       converted_audio_dir=output_dir_for(a.src, a.tgt, a.ckpt_type, a.post_opt, a.dur_limit),
                       required_subset_file=a.required_subset_file, duration_limit=a.dur_limit, **common)
        return 0
    raise SystemExit("Both inputs must be files or both must be folders.")


if __name__ == "__main__":
    raise SystemExit(main())
