"""The Python binding (_cabi.py, host_cpp_binding.py) seen from outside, without a GPU: its C signatures, public names, method
signatures and record layouts, and every C call its public methods make, equal what tests/golden/make_fixtures.py recorded from the
binding before its near-copies were folded together (cabi_surface.json, cabi_transcript.json; tests/cabi_record.py does the looking)."""
import inspect
import json
import os

import cabi_record

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def golden(name):
    return json.load(open(os.path.join(GOLDEN, name)))


def test_surface_is_the_recorded_one(rtx):
    got, want = json.loads(json.dumps(cabi_record.surface(rtx))), golden("cabi_surface.json")
    assert sorted(got) == sorted(want)
    for part in want:
        if isinstance(want[part], dict):
            assert sorted(got[part]) == sorted(want[part]), part
            for k in want[part]:
                assert got[part][k] == want[part][k], (part, k)
        assert got[part] == want[part], part


def test_every_public_method_is_driven(rtx):
    """the transcript leaves out no public method but those cabi_record.NOT_DRIVEN names, line by line, and they are few"""
    assert len(cabi_record.NOT_DRIVEN) <= 5
    driven = cabi_record.driven(golden("cabi_transcript.json"))
    for name, cls in (("Tracer", rtx.Tracer), ("MultiTracer", rtx.MultiTracer), ("CppScene", rtx.host_cpp_binding.CppScene)):
        methods = {n for n in dir(cls) if not n.startswith("_") and callable(inspect.getattr_static(cls, n))}
        missing = methods - driven[name] - {m for c, m in cabi_record.NOT_DRIVEN if c == name}
        assert not missing, (name, sorted(missing))


def test_calls_are_the_recorded_ones(rtx):
    got, want = json.loads(json.dumps(cabi_record.transcript(rtx))), golden("cabi_transcript.json")
    assert sorted(got) == sorted(want)
    for cls in want:
        assert [s["step"] for s in got[cls]] == [s["step"] for s in want[cls]], cls
        for g, w in zip(got[cls], want[cls]):
            assert g == w, (cls, w["step"])
        for s in got[cls]:
            assert s.get("zeroed", True), (cls, s["step"], "a host output that was not zero-initialised")
