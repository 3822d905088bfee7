"""CPU: options.Extensions, the one checked record of the extension knobs — the two constructors fold the calling conventions
to the same fields, refuse every bad value the per-knob tests list (test_topk_cpu.py, test_pitch_cpu.py, test_dynamics_cpu.py),
and the record cannot be changed afterwards."""
import dataclasses

import numpy as np
import pytest

from knn_svc_amd.options import Extensions

OFF = dict(topk=None, vad_level=0, loudness_db=None, envelope_mix=0.0, peak_db=None)

# knob: (its from_reference arguments with the switch OFF, the same with the switch ON, the from_serving arguments that mean ON)
SWITCHED = {
    "topk": (dict(topk=6, use_topk=False), dict(topk=6, use_topk=True), dict(topk=6)),
    "loudness": (dict(tgt_loudness_db=-23, normalize_loudness=False), dict(tgt_loudness_db=-23, normalize_loudness=True),
                 dict(loudness_db=-23)),
    "vad": (dict(vad_trigger_level=7, use_vad=False), dict(vad_trigger_level=7, use_vad=True), dict(vad_trigger_level=7)),
}
# the knobs without a switch: (from_reference arguments, from_serving arguments)
PLAIN = {
    "f0_shift": (dict(f0_shift="octave"), dict(f0_shift="octave", transpose=0.0)),
    "transpose": (dict(transpose=-2.5), dict(f0_shift="median", transpose=-2.5)),
    "envelope_mix": (dict(envelope_mix=0.5), dict(f0_shift="median", transpose=0.0, envelope_mix=0.5)),
    "peak_db": (dict(peak_db=-1), dict(f0_shift="median", transpose=0.0, peak_db=-1)),
}


def test_defaults_of_both_constructors_are_all_off():
    ref, srv = Extensions.from_reference(), Extensions.from_serving()
    assert srv == Extensions() and dataclasses.asdict(srv) == dict(OFF, f0_shift=None, transpose=None)
    assert dataclasses.asdict(ref) == dict(OFF, f0_shift="median", transpose=0.0)        # kept as given: upstream's names


@pytest.mark.parametrize("knob", sorted(SWITCHED))
def test_a_value_is_ignored_unless_its_switch_is_on(knob):
    off, on, serving = SWITCHED[knob]
    assert Extensions.from_reference(**off) == Extensions.from_reference()               # whatever the value
    got = Extensions.from_reference(**on)
    assert got != Extensions.from_reference()
    assert got == Extensions.from_serving(f0_shift="median", transpose=0.0, **serving)


def test_switched_values_off_are_not_even_checked():
    assert Extensions.from_reference(topk=99, tgt_loudness_db="loud", vad_trigger_level=None) == Extensions.from_reference()


@pytest.mark.parametrize("knob", sorted(PLAIN))
def test_unswitched_knobs_take_effect_as_passed_and_agree_between_the_constructors(knob):
    ref, serving = PLAIN[knob]
    got = Extensions.from_reference(**ref)
    assert got != Extensions.from_reference() and got == Extensions.from_serving(**serving)


def test_fields_hold_the_resolved_values():
    e = Extensions.from_serving(loudness_db=-20, topk=np.int64(3), vad_trigger_level=4.5, f0_shift="semitone", transpose=2,
                                envelope_mix=np.float32(0.5), peak_db=-1)
    assert dataclasses.asdict(e) == dict(topk=3, vad_level=4.5, f0_shift="semitone", transpose=2, loudness_db=-20.0,
                                         envelope_mix=0.5, peak_db=-1.0)
    assert type(e.topk) is int and type(e.loudness_db) is float and type(e.envelope_mix) is float and type(e.peak_db) is float
    every = Extensions.from_reference(topk=3, use_topk=True, tgt_loudness_db=-20, normalize_loudness=True, use_vad=True,
                                      vad_trigger_level=4.5, f0_shift="semitone", transpose=2, envelope_mix=0.5, peak_db=-1)
    assert every == e


# the bad values of the per-knob tests: test_topk_cpu.py:135, test_pitch_cpu.py:48-50, test_dynamics_cpu.py:148, 151
BAD = ([("topk", v) for v in (9, 0, -1, 2.5, True)]
       + [("f0_shift", v) for v in ("fifth", "Median", 4, 0, True)]
       + [("transpose", v) for v in (float("nan"), float("inf"), -float("inf"), 36.5, -37, True, False, "2", [1.0])]
       + [("envelope_mix", v) for v in (-0.01, 1.01, float("nan"), float("inf"), "0.5", True, [0.5])]
       + [("peak_db", v) for v in (0.1, float("nan"), float("inf"), float("-inf"), "-1", False, (-1,))])


@pytest.mark.parametrize("knob,value", BAD, ids=[f"{k}={v!r}" for k, v in BAD])
def test_both_constructors_refuse_a_bad_value(knob, value):
    with pytest.raises(ValueError):
        Extensions.from_serving(**{knob: value})
    with pytest.raises(ValueError):
        Extensions.from_reference(**{knob: value}, use_topk=True)


def test_the_record_is_frozen():
    e = Extensions.from_serving(topk=3)
    for field in dataclasses.fields(e):
        with pytest.raises(dataclasses.FrozenInstanceError):
            setattr(e, field.name, None)
    assert e == Extensions.from_serving(topk=3) and hash(e) == hash(Extensions.from_serving(topk=3))
